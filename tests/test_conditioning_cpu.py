"""The ill-conditioned inputs of tests/conditioning_ref.py do their job, and the fp64 references are sound on them (no GPU).

  (a) a one-pass fp32 `E[x^2] - mean^2` in the summation order of gn_stats_kernel misses the rstd bar of the GPU tests on the inputs whose
      mean dominates -- the tests discriminate;
  (b) the same single pass about a per-channel pivot meets it on every case -- the bar can be met without a second pass over x;
  (c) under attn128_fwd's lazy-maximum policy every softmax case sends a good share of the query rows through the rescale branch after
      the first key tile, and leaves a good share on a stale reference;
  (d) the plain randn input does not (why the older tests never covered the branch), and rows that saturate keep a finite reference."""
import pytest
import torch

import conditioning_ref as CR


@pytest.mark.parametrize("P,C,G", CR.GN_SHAPES)
@pytest.mark.parametrize("name", CR.GN_CASES)
def test_groupnorm_one_pass_fp32_misses_and_shifted_meets_the_bar(name, P, C, G):
    c = CR.gn_case(name, P, C, G)
    ref = CR.gn_reference(name, P, C, G)
    _, rstd_naive = CR.gn_stats_naive_fp32(c["x"], G, c["eps"])
    mean_s, rstd_s = CR.gn_stats_shifted_fp32(c["x"], G, c["eps"])
    miss_naive = CR.stat_miss(rstd_naive, ref["rstd"], CR.GN_STAT_RTOL)
    miss_shift = CR.stat_miss(rstd_s, ref["rstd"], CR.GN_STAT_RTOL)
    miss_mean = CR.stat_miss(mean_s, ref["mean"], CR.GN_STAT_RTOL, CR.GN_STAT_ATOL_MEAN)
    print(f"[{name} P={P} C={C} G={G}] rstd error / bar: one-pass {miss_naive:.3g}, shifted {miss_shift:.3g}; shifted mean {miss_mean:.3g}")
    if name in CR.GN_ILL or name == "two_samples":                   # two_samples: sample 0 is a plateau
        assert miss_naive > 1.0, "the input does not break a one-pass fp32 variance: the GPU test on it proves nothing"
    if name in ("plateau", "plateau_small"):
        # not one unlucky group: the sums of x^2 (~ 1e4 P) carry an fp32 spacing of the order of the variance itself, so a group lands
        # within 1e-4 of the truth only by chance -- most groups must miss
        rel = (torch.as_tensor(rstd_naive).double() / ref["rstd"] - 1).abs()
        print(f"    per-group rstd error: smallest {rel.min().item():.3g}, median {rel.median().item():.3g}, largest {rel.max().item():.3g}")
        assert rel.median().item() > CR.GN_STAT_RTOL, rel.median().item()
    assert miss_shift <= 1.0 and miss_mean <= 1.0


def test_groupnorm_two_samples_statistics_are_per_sample():
    P, C, G = CR.GN_SHAPES[0]
    ref = CR.gn_reference("two_samples", P, C, G)
    assert ref["var"][0].max().item() < 0.01 and ref["var"][1].min().item() > 0.9        # a plateau next to randn
    assert ref["mean"][0].min().item() > 99 and ref["mean"][1].abs().max().item() < 0.1


def test_groupnorm_constant_group_has_zero_variance_and_finite_reference():
    P, C, G = CR.GN_SHAPES[1]
    c = CR.gn_case("constant_group", P, C, G)
    ref = CR.gn_reference("constant_group", P, C, G)
    assert ref["var"][0, 1].item() == 0.0 and ref["rstd"][0, 1].item() == pytest.approx(c["eps"] ** -0.5)
    assert CR.finite(ref["y"], ref["dx"], ref["dgamma"], ref["dbeta"])


SOFTMAX_RUNS = [(1, 333, 2, None), (1, 333, 2, (300,)), (2, 333, 2, (333, 137))]


@pytest.mark.parametrize("B,S,H,lens", SOFTMAX_RUNS, ids=["full", "kv300", "b2"])
@pytest.mark.parametrize("name", CR.SOFTMAX_CASES)
def test_softmax_cases_reach_the_rescale_branch_and_a_stale_reference(name, B, S, H, lens):
    cov = CR.lazy_max_coverage(CR.softmax_qkv(name, B, S, H), H, lens)
    print(f"[{name} B={B} S={S} H={H} kv_len={lens}] {cov}")
    assert cov["rescaled"] >= 0.05 * cov["rows"], cov
    assert cov["stale"] >= 0.05 * cov["rows"] and 0 < cov["max_rise"] <= CR.LAZY_THRESHOLD, cov


def test_plain_randn_never_takes_the_rescale_branch_after_the_first_tile():
    """the input of test_attn128_matches_dense_attention: why that test alone does not cover the branch"""
    cov = CR.lazy_max_coverage(CR.softmax_qkv("randn", 1, 333, 2), 2, None)
    print(f"[randn] {cov}")
    assert cov["rescaled"] < 0.05 * cov["rows"], cov


def test_masked_spike_key_moves_nothing():
    """late_spike at kv_len = 300: key 330 (x 12) is masked, so fewer rows rescale than without the mask, and the reference ignores it"""
    qkv = CR.softmax_qkv("late_spike", 1, 333, 2)
    full = CR.lazy_max_coverage(qkv, 2, None); cut = CR.lazy_max_coverage(qkv, 2, (300,))
    assert cut["rescaled"] < full["rescaled"]
    _, _, s, _ = CR.dense_attention64(qkv, 2, (300,))
    assert bool(torch.isinf(s[..., 330]).all())


def test_masked_giant_key_would_underflow_fp32_if_it_moved_the_reference():
    """a masked x 12 key that wrongly moved the running reference would cost nothing: exp2 of the valid scores stays within fp32's range and
    the final division restores them -- and late_spike's key 330 lies in a key tile that kv_len = 300 keeps the kernels from loading at
    all.  Key 301 x 150 is inside the last loaded 64-key tile (256 .. 319), and for a good share of the rows its score lies more than 126
    log2 units (the smallest normal fp32 is 2^-126) above every valid key's: a kernel that lets it move the reference returns zeros there."""
    B, S, H = 1, 333, 2
    at = S - 32
    assert 300 <= at < 64 * ((300 + 63) // 64)
    qkv = CR.softmax_qkv("masked_giant", B, S, H)
    _, _, s_open, _ = CR.dense_attention64(qkv, H, None)
    o, lse2, s, _ = CR.dense_attention64(qkv, H, (300,))
    lead = (s_open[..., at] - s[..., :300].max(-1).values) * CR.LOG2E
    n = int((lead > 126).sum())
    print(f"[masked_giant] {n} of {lead.numel()} rows: the masked key leads by more than 126 log2 units")
    assert n >= 0.05 * lead.numel()
    assert bool(torch.isinf(s[..., at]).all()) and CR.finite(o, lse2)
    cov = CR.lazy_max_coverage(qkv, H, (300,))
    assert cov["rescaled"] < 0.05 * cov["rows"], cov                  # under the kernel's policy the masked key moves nothing


@pytest.mark.parametrize("name", ["late_spike", "staircase"])         # the constructions with single leading keys
def test_saturated_softmax_rows_have_a_finite_fp64_reference(name):
    """the same constructions ten times steeper: rows where one key leads by more than 100 nats.  Output, log-sum-exp and all three
    gradients of the dense fp64 reference stay finite there (softmax subtracts the row maximum first)."""
    B, S, H = 1, 333, 2
    qkv = CR.softmax_qkv(name, B, S, H, mult=10.0)
    g = torch.randn(B, S, H * 128, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16)
    o, lse2, s, dqkv = CR.dense_attention64(qkv, H, None, g)
    sat = CR.saturated_rows(s)
    print(f"[{name} x 10] {int(sat.sum())} of {sat.numel()} rows saturate")
    assert int(sat.sum()) >= 0.05 * sat.numel()
    assert CR.finite(o, lse2, dqkv)
    assert dqkv.abs().max().item() > 0
