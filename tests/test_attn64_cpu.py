"""CPU: do the inputs of tests/test_attn64_gpu.py reach the code they aim at?  Checked on the fp64 reference and on the restated lazy-maximum
policy of the hd64 forward alone (tests/attn64_ref.py); no kernel runs here."""
import pytest
import torch

import attn64_ref as R
from conditioning_ref import SOFTMAX_CASES, finite

B, H, S = 1, 2, 333                                   # 6 key tiles, 11 waves per head
VARIANTS = ("m32", "m16")


def _policy(name, variant, shape=(B, S, H)):
    b, s, h = shape
    return R.lazy_policy64(R.qkv_case(name, b, s, h, True)[0], h, variant)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", SOFTMAX_CASES)
def test_every_family_rescales_after_tile_0_in_every_wave(name, variant):
    p = _policy(name, variant)
    assert p["tiles"] == 6 and p["waves"] == 22
    assert p["rescaled_waves"] == p["waves"], (p["rescaled_waves"], p["waves"])
    assert p["stale_rows"] > 0 and 0.0 < p["max_stale_rise"] <= R.LAZY_THR, (p["stale_rows"], p["max_stale_rise"])


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_families_together_rescale_at_every_tile_position(variant):
    tiles = set()
    for name in SOFTMAX_CASES:
        tiles |= _policy(name, variant)["rescale_tiles"]
    assert tiles == set(range(1, 6)), tiles


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", [(1, 333, 2), (2, 193, 3), (2, 257, 3)])
def test_plain_randn_never_rescales_after_tile_0(shape, variant):
    p = _policy("randn", variant, shape)
    assert p["rescaled_waves"] == 0 and p["rescale_tiles"] == set()


@pytest.mark.parametrize("s,tiles", [(65, set()), (67, {1}), (129, {1}), (131, {1, 2}), (193, {1, 2})])
def test_late_spike_around_a_ragged_tile(s, tiles):
    """where late_spike rescales at the sizes whose last tile holds one key (65, 129, 193) or three keys led by the x 12 key (67, 131):
    most waves rescale (a wave does when one of its 32 rows rises by more than 8), except at 65, where both scaled keys are in tile 0"""
    p = _policy("late_spike", "m32", (2, s, 3))
    assert p["rescale_tiles"] == tiles
    assert 2 * p["rescaled_waves"] > p["waves"] or not tiles


@pytest.mark.parametrize("name", ("randn",) + SOFTMAX_CASES)
def test_lane_grouping_does_not_change_the_policy(name):
    """a wave rescales when any lane's partial maximum rises by more than 8, i.e. when some row's maximum does: two or four lane groups
    give the same references.  (What differs between the kernels is the exchange a wrong build can get wrong.)"""
    a, b = _policy(name, "m32"), _policy(name, "m16")
    assert torch.equal(a["m_final"], b["m_final"]) and a["rescale_tiles"] == b["rescale_tiles"]


def test_final_reference_is_at_most_8_below_the_row_maximum():
    for name in SOFTMAX_CASES:
        dev = R.qkv_case(name, B, S, H, True)[0].double()
        smax = torch.einsum("bqhd,bkhd->bhqk", dev[:, :, 0], dev[:, :, 1]).max(-1).values
        gap = smax - _policy(name, "m32")["m_final"]
        assert bool((gap <= R.LAZY_THR).all()), gap.max()


def test_prescaled_q_is_bf16_and_the_reference_sees_it():
    dev, ref = R.qkv_case("staircase", 1, 65, 2, True)
    assert torch.equal(dev, dev.to(torch.bfloat16).float())
    assert torch.equal(ref[:, :, 0], dev[:, :, 0].double() / R.SC2) and torch.equal(ref[:, :, 1:], dev[:, :, 1:].double())
    plain, ref0 = R.qkv_case("staircase", 1, 65, 2, False)
    assert torch.equal(ref0, plain.double()) and torch.equal(plain[:, :, 1:], dev[:, :, 1:])


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("name,b,s,h", R.all_cases())
def test_reference_is_finite_and_not_degenerate(name, b, s, h, pre):
    r = R.reference(name, b, s, h, pre)
    assert finite(r["o"], r["lse2"], r["dqkv"])
    assert r["degenerate"] == 0
    assert r["dqkv"].abs().max().item() > 0 or s == 1          # one key: softmax is constant, dq = dk = 0 exactly


def test_chain_cases_are_stated_as_the_kernel_schedules_them():
    """the hand-written plans against the scheduling rules in words (attn64_ref.CHAIN_CASES): grid = items rounded up to 8 or the slot knob,
    chain length bounded by grid / 8 and by the key blocks of a head, generations = items over grid rounded up"""
    for name, (b, h, s, L, slots, (eL, eg, egen)) in R.CHAIN_CASES.items():
        nkb = -(-s // 256)
        items = nkb * h * b
        assert eg % 8 == 0 and (eg == slots if slots else eg - 8 < items <= eg), name
        assert eL == (L or 3) and 1 < eL <= eg // 8 and eL <= nkb, name
        assert egen == -(-items // eg), name


def _scores2(name, b, s, h):
    dev = R.qkv_case(name, b, s, h, True)[0].double()
    return torch.einsum("bqhd,bkhd->bhqk", dev[:, :, 0], dev[:, :, 1])               # log2 units


@pytest.mark.parametrize("s", [31, 67])
def test_all_low_puts_every_real_score_far_below_the_masked_zeros(s):
    """below -150 log2 units, the smallest fp32 exp2 can return: a reference at 0 (the score of a key past S before its mask) loses every row;
    and the rows are no one-hot softmax"""
    sc = _scores2("all_low", 2, s, 3)
    assert sc.max().item() < -150.0
    top = sc.topk(2, dim=-1).values
    assert (top[..., 0] - top[..., 1]).max().item() < 30.0
    r = R.reference("all_low", 2, s, 3, True)
    assert finite(r["o"], r["lse2"])


def test_early_giant_has_rows_a_lowered_reference_would_overflow():
    """some wave rescales at tile 1 (a row of it rises by more than 8) while another of its rows holds a reference more than 128 log2 units
    above its own tile-1 maximum: lowering that row's reference to the tile maximum multiplies its accumulators by exp2(128 ..)"""
    b, s, h = 2, 129, 3
    p = R.lazy_policy64(R.qkv_case("early_giant", b, s, h, True)[0], h)
    assert 1 in p["rescale_tiles"]
    sc = _scores2("early_giant", b, s, h)
    ref0 = sc[..., :64].max(-1).values                                                 # the reference after tile 0
    t1 = sc[..., 64:128].max(-1).values
    rows = torch.arange(-(-s // 32) * 32).clamp_max(s - 1)
    rise = (t1 - ref0)[..., rows].view(b, h, -1, 32)
    both = ((rise > R.LAZY_THR).any(-1)) & ((rise < -128.0).any(-1))
    assert int(both.sum()) >= 3, int(both.sum())
    r = R.reference("early_giant", b, s, h, True)
    assert finite(r["o"], r["lse2"])
