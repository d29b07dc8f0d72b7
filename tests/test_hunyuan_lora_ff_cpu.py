"""HunyuanVideo LoRA feed-forward targets (lora_target_modules: ff.net.0.proj, ff.net.2, proj_mlp, proj_out) without a device: target
resolution and refusals, parameter names / shapes / flat order, the default targets' unchanged parameter list, the LoRA-only state-dict
round trip, and the floor-derived gradient bars (parity.floor_bars) on the fp64 oracle and its bf16 restatement with all eight targets."""
import os
import sys

import pytest
import torch

from hunyuan_lora_ff_ref import ALL, ATTN, FF, blocks_loss, golden, init_adapters, lora_effective
from parity import floor_bars, grad_floor, grad_report

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import hunyuan_oracle as HO              # noqa: E402

BF = torch.bfloat16
KW = dict(hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_alpha=2.0)

# named_parameters() of the adapters of a 1 + 1 block model on the parent commit, written out
PARENT_NAMES = [
    "lora.double_blocks.0.img_attn_qkv.lora_A.q.weight", "lora.double_blocks.0.img_attn_qkv.lora_A.k.weight",
    "lora.double_blocks.0.img_attn_qkv.lora_A.v.weight", "lora.double_blocks.0.img_attn_qkv.lora_B.q.weight",
    "lora.double_blocks.0.img_attn_qkv.lora_B.k.weight", "lora.double_blocks.0.img_attn_qkv.lora_B.v.weight",
    "lora.double_blocks.0.img_attn_proj.lora_A.weight", "lora.double_blocks.0.img_attn_proj.lora_B.weight",
    "lora.single_blocks.0.linear1.lora_A.q.weight", "lora.single_blocks.0.linear1.lora_A.k.weight",
    "lora.single_blocks.0.linear1.lora_A.v.weight", "lora.single_blocks.0.linear1.lora_B.q.weight",
    "lora.single_blocks.0.linear1.lora_B.k.weight", "lora.single_blocks.0.linear1.lora_B.v.weight"]
# the flat buffer's order on the parent commit: A then B per adapter, module by module
PARENT_FLAT = [f"double_blocks.0.img_attn_qkv.lora_{ab}.{t}.weight" for t in "qkv" for ab in "AB"] + \
              ["double_blocks.0.img_attn_proj.lora_A.weight", "double_blocks.0.img_attn_proj.lora_B.weight"] + \
              [f"single_blocks.0.linear1.lora_{ab}.{t}.weight" for t in "qkv" for ab in "AB"]
# the feed-forward sites' parameters, behind them (D 256, 4D 1024, D + 4D 1280)
FF_FLAT = {"ff.net.0.proj": [("double_blocks.0.img_mlp.fc1.lora_A.weight", 256), ("double_blocks.0.img_mlp.fc1.lora_B.weight", 1024)],
           "ff.net.2": [("double_blocks.0.img_mlp.fc2.lora_A.weight", 1024), ("double_blocks.0.img_mlp.fc2.lora_B.weight", 256)],
           "proj_mlp": [("single_blocks.0.linear1.lora_A.mlp.weight", 256), ("single_blocks.0.linear1.lora_B.mlp.weight", 1024)],
           "proj_out": [("single_blocks.0.linear2.lora_A.weight", 1280), ("single_blocks.0.linear2.lora_B.weight", 256)]}


def _blocks(**kw):
    from vt355.hunyuan import HunyuanBlocks
    return HunyuanBlocks(**{**KW, **kw})


def test_target_resolution_and_refusals():
    from vt355.hunyuan import resolve_lora_targets
    assert resolve_lora_targets(None) == (True, ())
    assert resolve_lora_targets(list(ATTN)) == (True, ())
    assert resolve_lora_targets(list(reversed(ALL))) == (True, FF)                     # FF order, whatever the order given
    assert resolve_lora_targets(["proj_out"]) == (False, ("proj_out",))
    assert resolve_lora_targets(["ff.net.2", "ff.net.0.proj"]) == (False, ("ff.net.0.proj", "ff.net.2"))
    assert resolve_lora_targets("proj_mlp") == (False, ("proj_mlp",))
    for part in (["to_q"], ["to_q", "to_k", "to_v"], ["to_out.0", "proj_out"], ["to_k", "to_v", "to_out.0", "ff.net.2"]):
        with pytest.raises(ValueError, match="together"):
            resolve_lora_targets(part)
    for bad in (["to_out"], ["ff.net.0"], ["fc1"], ["linear2"], ["proj"], ["to_q", "to_k", "to_v", "to_out.0", "mlp"]):
        with pytest.raises(ValueError, match="unsupported"):
            resolve_lora_targets(bad)
    with pytest.raises(ValueError):
        resolve_lora_targets([])
    # the constructors refuse the same way, with or without a rank
    with pytest.raises(ValueError, match="unsupported"):
        _blocks(lora_rank=4, lora_target_modules=["norm"])
    with pytest.raises(ValueError, match="together"):
        _blocks(lora_rank=0, lora_target_modules=["to_q"])


def test_default_targets_are_the_parent_commits_parameters():
    """None and the four attention names: named_parameters(), the flat order and every offset are what they were"""
    for tm in (None, list(ATTN)):
        m = _blocks(lora_rank=4, lora_target_modules=tm)
        assert [n for n, _ in m.named_parameters() if n.startswith("lora.")] == PARENT_NAMES
        assert list(m.lora.shapes) == PARENT_FLAT
        assert m.lora.numel == 14 * 4 * 256 and [m.lora.offsets[n] for n in PARENT_FLAT] == [i * 4 * 256 for i in range(14)]
        assert not m.lora.ff and m.lora.attn


@pytest.mark.parametrize("r", [4, 24, 128])
def test_parameter_names_shapes_and_order(r):
    m = _blocks(lora_rank=r, lora_target_modules=list(ALL))
    names = list(m.lora.shapes)
    assert names[:14] == PARENT_FLAT                                                   # the new parameters come behind the existing ones
    assert names[14:] == [n for t in FF for n, _ in FF_FLAT[t]]
    for t in FF:
        (na, K), (nb, N) = FF_FLAT[t]
        assert m.lora.shapes[na] == (r, K) and m.lora.shapes[nb] == (N, r)
        assert m.lora.offsets[na] >= 14 * r * 256
    sd = m.state_dict()
    for n in names:
        assert tuple(sd["lora." + n].shape) == m.lora.shapes[n]
    # every target on its own, and the feed-forward ones without the attention group: what is not requested does not exist
    for t in FF:
        one = _blocks(lora_rank=r, lora_target_modules=[t])
        assert list(one.lora.shapes) == [n for n, _ in FF_FLAT[t]] and not one.lora.sites
    ffonly = _blocks(lora_rank=r, lora_target_modules=list(FF))
    assert list(ffonly.lora.shapes) == names[14:]
    # two blocks of each kind: block by block, fc1 before fc2, linear1's mlp adapter before linear2
    m2 = _blocks(lora_rank=r, lora_target_modules=list(FF), mm_double_blocks_depth=2, mm_single_blocks_depth=2)
    mods = [n.split(".lora_")[0] for n in list(m2.lora.shapes)[::2]]
    assert mods == ["double_blocks.0.img_mlp.fc1", "double_blocks.0.img_mlp.fc2", "double_blocks.1.img_mlp.fc1", "double_blocks.1.img_mlp.fc2",
                    "single_blocks.0.linear1", "single_blocks.0.linear2", "single_blocks.1.linear1", "single_blocks.1.linear2"]


def test_whole_model_and_flow_pass_the_targets_through():
    from vt355.hunyuan import HunyuanVideoFlow, HYVideoDiffusionTransformer
    kw = dict(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1, text_states_dim=64,
              text_states_dim_2=32, lora_rank=8, lora_alpha=2.0)
    m = HYVideoDiffusionTransformer(lora_target_modules=list(ALL), **kw)
    assert list(m.lora.shapes)[14:] == [n for t in FF for n, _ in FF_FLAT[t]]
    # the refiner's feed-forward and the final layer stay frozen: no adapter is named after them
    assert not any(n.startswith(("txt_in.", "final_layer.")) for n in m.lora.shapes)
    assert list(HYVideoDiffusionTransformer(**kw).lora.shapes) == PARENT_FLAT
    flow = HunyuanVideoFlow(denoiser_config={"target": "vt355.hunyuan.HYVideoDiffusionTransformer",
                                             "params": {**kw, "lora_target_modules": ["to_q", "to_k", "to_v", "to_out.0", "proj_out"]}})
    assert list(flow.model.lora.shapes)[14:] == [n for n, _ in FF_FLAT["proj_out"]]


def test_lora_only_state_dict_round_trip():
    """the reference's LoRA-only checkpoint filter (the substring "lora") keeps exactly the adapters, the new ones included, and a fresh
    model loads them back bit for bit"""
    m = _blocks(lora_rank=24, lora_target_modules=list(ALL))
    m.init_weights(1)
    m.lora.init_weights(7, zero_b=False)
    only = {k: v.clone() for k, v in m.state_dict().items() if "lora" in k}
    assert sorted(only) == sorted("lora." + n for n in m.lora.shapes) and len(only) == 22
    m2 = _blocks(lora_rank=24, lora_target_modules=list(ALL))
    missing, unexpected = m2.load_state_dict(only, strict=False)
    assert not unexpected and not any("lora" in k for k in missing)
    for n in m.lora.shapes:
        assert torch.equal(m2.lora._plist[n].detach(), m.lora._plist[n].detach()) and m2.lora._plist[n].abs().max() > 0, n
    # a model with fewer targets refuses the extra keys under strict loading
    m3 = _blocks(lora_rank=24)
    with pytest.raises(RuntimeError):
        m3.load_state_dict({**{k: v for k, v in m.state_dict().items()}}, strict=True)


def test_floor_bars_with_all_eight_targets():
    """in the style of tests/test_grad_bars_cpu.py: one double and one single block on tests/golden/hunyuan_blocks.npz with rank-4 adapters on
    all eight targets (adapters alone trained).  The bf16 restatement of the oracle passes the floor-derived bars against fp64 with no
    parameter flagged; the same model with the ff.net.2 adapter's scaling taken for rank r + 1 is flagged on that adapter."""
    T = golden()
    D, H, M4, r, alpha = 256, 2, 1024, 4, 2.0
    base = {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}
    base = {k: v.to(BF) for k, v in base.items()}
    ad0 = {k: v.to(BF) for k, v in init_adapters(ALL, D, M4, r).items()}
    img, txt, vec = [T(k).to(BF) for k in ("img", "txt", "vec")]
    tv, gx = T("txt_valid"), T("s_gx").to(BF)

    def grads(dt, scaling_of=None):
        ad = {k: v.detach().to(dt).requires_grad_(True) for k, v in ad0.items()}
        Pe = lora_effective({k: v.to(dt) for k, v in base.items()}, ad, ALL, alpha / r, D, M4, scaling_of=scaling_of)
        cos, sin = (T("cos").double(), T("sin").double()) if dt == torch.float64 else (T("cos"), T("sin"))
        out, loss = blocks_loss(HO, Pe, img.to(dt), txt.to(dt), vec.to(dt), tv, cos, sin, gx, H)
        assert out.dtype == dt
        loss.backward()
        return {k: v.grad for k, v in ad.items()}

    ref, noisy = grads(torch.float64), grads(BF)
    assert len(ref) == 22 and all(g.dtype == BF for g in noisy.values())
    floor, ofloor = grad_floor(noisy, ref)
    bars = floor_bars(floor, 0.2)
    pairs = lambda d: [(n, d[n], ref[n]) for n in ref]
    overall, worst, bad = grad_report(pairs(noisy), 0.98, bars)
    fl = sorted(floor.values())
    print(f"[hunyuan lora ff] 22 adapters; bf16 floor median {fl[11]:.2e}, worst {fl[-1]:.2e}, overall {ofloor:.2e}")
    assert not bad, bad
    assert grad_report(pairs(ref), 0.98, bars)[1] == 0.0
    wrong = grads(BF, scaling_of={"ff.net.2": alpha / (r + 1)})
    _, worst_w, bad_w = grad_report(pairs(wrong), 0.98, bars)
    flagged = {b[0] for b in bad_w}
    print(f"[hunyuan lora ff] ff.net.2 scaling alpha / (r + 1): worst rel-L2 {worst_w:.3f}, flagged {sorted(flagged)}")
    assert {"double_blocks.0.img_mlp.fc2.lora_A.weight", "double_blocks.0.img_mlp.fc2.lora_B.weight"} <= flagged
