"""tests/parity.py on the CPU: the comparators accept an fp64 reference against its own bf16 rounding at the tightest limits the suite
uses and reject every mutation a wrong kernel produces (NaN, Inf, one element out of tolerance, a zeroed or sign-flipped gradient); the
idioms they replaced are kept here, frozen, to show that those accepted the NaN mutations; poisoned buffers round-trip their bits and
`untouched` sees one element written outside the region; and the GPU test sources define no comparator of their own and allocate no
kernel output with torch.empty."""
import ast
import glob
import math
import os
import re

import pytest
import torch

import parity
from parity import all_written, close, floor_bars, floor_report, grad_floor, grad_report, is_poison, overall_bar, poisoned, poisoned_like, rel_l2, relerr, untouched

BF = torch.bfloat16
HERE = os.path.dirname(os.path.abspath(__file__))
# the tightest limits of the suite for a bf16 output: rtol 8e-3 (sinusoid golden), atol 1e-3 (AdamW's bf16 copy); rel-L2 5e-3 (fp8 GEMM);
# cosine 0.99 / rel-L2 0.15 per parameter (full fine-tune).  bf16 rounds to nearest with 8 significant bits: |err| <= 2^-8 |ref|
RTOL, ATOL, REL_MAX, COS_MIN, GREL_MAX = 8e-3, 1e-3, 5e-3, 0.99, 0.15


# ------------------------------------------------------------------ the replaced idioms, frozen
def old_close_passes(a, b, rtol, atol):
    a = a.detach().float().cpu(); b = b.detach().float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    return bad == 0.0


def old_grad_loop(pairs, cos_min, rel_max):
    bad, worst = [], 0.0
    for n, gd, gr in pairs:
        e, d = (gd - gr).norm().item(), gr.norm().item()
        cos = torch.nn.functional.cosine_similarity(gd.flatten(), gr.flatten(), dim=0).item()
        worst = max(worst, e / max(d, 1e-12))
        if cos < cos_min or e / max(d, 1e-12) > rel_max:
            bad.append((n, e / max(d, 1e-12), cos))
    return worst, bad


@pytest.fixture(scope="module")
def pair():
    g = torch.Generator().manual_seed(1)
    ref = torch.randn(1000, 1000, generator=g, dtype=torch.float64) * 3.0          # 10^6 elements
    return ref, ref.to(BF)


def _mutations(ref, got):
    n = ref.numel()
    out = {}
    out["all NaN"] = torch.full_like(got, float("nan"))
    m = got.clone(); m.view(-1)[n // 3] = float("nan"); out["one NaN in 10^6"] = m
    m = got.clone(); m.view(-1)[n - 1] = float("inf"); out["one +Inf"] = m
    m = got.clone(); m.view(-1)[0] = float("-inf"); out["one -Inf"] = m
    i = 777_777
    m = got.double().clone(); m.view(-1)[i] = ref.view(-1)[i] + 2 * (ATOL + RTOL * ref.view(-1)[i].abs()); out["one element off by 2 tol"] = m
    return out


def test_close_accepts_bf16_rounding_and_rejects_every_mutation(pair):
    ref, got = pair
    close(got, ref, RTOL, ATOL, "bf16 rounding")
    close(got, ref, RTOL, 0.0, "bf16 rounding, relative only")
    for name, m in _mutations(ref, got).items():
        with pytest.raises(AssertionError, match="out of tol"):
            close(m, ref, RTOL, ATOL, name)
    # the message names the worst element and counts the non-finite ones
    m = got.clone(); m.view(-1)[123] = float("nan"); m.view(-1)[456] = float("inf")
    with pytest.raises(AssertionError, match=r"flat index (123|456)\b.*2 non-finite"):
        close(m, ref, RTOL, ATOL, "two")
    m = got.double().clone(); m.view(-1)[999] += 1.0
    with pytest.raises(AssertionError, match=r"0\.0001% out of tol, max err (0\.99|1).*ref absmax.*flat index 999\b.*0 non-finite"):
        close(m, ref, RTOL, ATOL, "one")
    # exact comparison (rtol = atol = 0) and an empty tensor
    close(got, got.double(), 0, 0, "exact")
    close(torch.zeros(0), torch.zeros(0), 0, 0, "empty")
    with pytest.raises(AssertionError, match="shape"):
        close(got[:10], ref, RTOL, ATOL, "shape")


def test_a_non_finite_reference_is_a_test_bug(pair):
    ref, got = pair
    for bad in (float("nan"), float("inf")):
        r = ref.clone(); r[0, 0] = bad
        with pytest.raises(ValueError, match="reference"):
            close(got, r, RTOL, ATOL, "ref")
        with pytest.raises(ValueError, match="ref"):
            rel_l2(got, r)
        with pytest.raises(ValueError, match="reference"):
            grad_report([("w", got, r)], COS_MIN, GREL_MAX)


def test_the_old_comparison_accepted_nan(pair):
    """why `(err > tol).float().mean()` is gone: NaN > tol is False"""
    ref, got = pair
    assert old_close_passes(got, ref, RTOL, ATOL)
    muts = _mutations(ref, got)
    assert old_close_passes(muts["all NaN"], ref, RTOL, ATOL)
    assert old_close_passes(muts["one NaN in 10^6"], ref, RTOL, ATOL)
    assert old_close_passes(torch.full((4, 4), float("nan")), torch.randn(4, 4), 1e-2, 1e-2)
    assert not old_close_passes(muts["one element off by 2 tol"], ref, RTOL, ATOL)          # it did see finite errors


def test_rel_l2_accepts_bf16_rounding_and_refuses_non_finite_input(pair):
    ref, got = pair
    e = rel_l2(got, ref)
    assert 0 < e < REL_MAX and e < 2.0 ** -8
    l2, mx = relerr(got, ref)
    assert l2 == pytest.approx(e) and 0 < mx < 2.0 ** -8
    assert rel_l2(ref, ref) == 0.0
    muts = _mutations(ref, got)
    for name in ("all NaN", "one NaN in 10^6", "one +Inf", "one -Inf"):
        with pytest.raises(AssertionError, match="non-finite"):
            rel_l2(muts[name], ref)
        with pytest.raises(AssertionError, match="non-finite"):
            relerr(muts[name], ref)
        with pytest.raises(AssertionError, match="non-finite"):
            parity.cosine(muts[name], ref)
    assert parity.cosine(got, ref) > 0.99999
    assert rel_l2(-got, ref) > 1.9


def _grads():
    g = torch.Generator().manual_seed(2)
    shapes = {"a.weight": (64, 48), "a.bias": (64,), "b.weight": (16, 64), "norm.weight": (64,)}
    ref = {n: torch.randn(s, generator=g, dtype=torch.float64) * 0.1 for n, s in shapes.items()}
    return ref, {n: r.to(BF) for n, r in ref.items()}


def test_grad_report_accepts_bf16_rounding_and_rejects_every_mutation():
    ref, got = _grads()
    pairs = lambda d: [(n, d[n], ref[n]) for n in ref]
    overall, worst, bad = grad_report(pairs(got), COS_MIN, GREL_MAX)
    assert not bad and 0 < overall <= worst < 2.0 ** -8
    # one parameter's gradient all NaN / one NaN / one Inf: refused by name
    for val in (float("nan"), float("inf")):
        m = dict(got); m["b.weight"] = torch.full_like(got["b.weight"], val)
        with pytest.raises(AssertionError, match=r"b\.weight: 1024 non-finite"):
            grad_report(pairs(m), COS_MIN, GREL_MAX)
        m = dict(got); t = got["a.bias"].clone(); t[5] = val; m["a.bias"] = t
        with pytest.raises(AssertionError, match=r"a\.bias: 1 non-finite"):
            grad_report(pairs(m), COS_MIN, GREL_MAX)
    # all zero: cosine 0, rel-L2 1
    m = dict(got); m["norm.weight"] = torch.zeros_like(got["norm.weight"])
    _, worst, bad = grad_report(pairs(m), COS_MIN, GREL_MAX)
    assert [b[0] for b in bad] == ["norm.weight"] and worst == pytest.approx(1.0)
    # sign-flipped: cosine -1, rel-L2 2
    m = dict(got); m["a.weight"] = -got["a.weight"]
    _, worst, bad = grad_report(pairs(m), COS_MIN, GREL_MAX)
    assert [b[0] for b in bad] == ["a.weight"] and bad[0][2] < -0.99 and worst == pytest.approx(2.0, rel=1e-2)
    # a missing gradient, a wrong size, nothing to compare
    with pytest.raises(AssertionError, match="no device gradient"):
        grad_report([("w", None, ref["a.bias"])], COS_MIN, GREL_MAX)
    with pytest.raises(AssertionError, match="elements"):
        grad_report([("w", got["a.bias"][:5], ref["a.bias"])], COS_MIN, GREL_MAX)
    with pytest.raises(AssertionError, match="no gradients"):
        grad_report([], COS_MIN, GREL_MAX)
    # the device gradient may live in another shape (a view of the flat buffer): both sides are flattened
    assert not grad_report([("w", got["a.weight"].reshape(-1), ref["a.weight"])], COS_MIN, GREL_MAX)[2]


def test_grad_report_thresholds_are_strict_and_nan_figures_are_bad():
    """`cos > cos_min and rel < rel_max`: a figure AT the limit is bad, and so is one that is NaN (overflowing finite values)"""
    r = torch.tensor([1.0, 0.0], dtype=torch.float64)
    _, _, bad = grad_report([("w", torch.tensor([1.0, 0.0]), r)], 1.0, 0.5)             # cos == 1.0 is not > 1.0
    assert bad
    _, _, bad = grad_report([("w", torch.tensor([1.5, 0.0]), r)], 0.5, 0.5)             # rel == 0.5 is not < 0.5
    assert bad
    assert not grad_report([("w", torch.tensor([1.25, 0.0]), r)], 0.5, 0.5)[2]
    huge = torch.full((4,), 1e200, dtype=torch.float64)
    _, worst, bad = grad_report([("ok", r.clone(), r), ("w", huge, -huge)], 0.5, 0.5)    # |gd - gr|^2 overflows: rel = inf / inf
    assert bad and bad[0][0] == "w" and (math.isnan(worst) or math.isinf(worst))


def test_grad_report_keeps_the_angle_of_a_tiny_gradient():
    """a gradient whose norm is far below 1 (a key bias: the softmax is shift-invariant, only rounding noise times the weights is left)
    is compared by its direction like any other: cosine_similarity clamps each norm at 1e-8 on its own, not their product"""
    g = torch.Generator().manual_seed(3)
    r = torch.randn(1920, generator=g, dtype=torch.float64) * 1e-7                  # |r| ~ 4e-6, |r|^2 ~ 2e-11 < 1e-8
    overall, worst, bad = grad_report([("to_k.bias", (r * 1.03).float(), r)], COS_MIN, GREL_MAX)
    assert not bad and worst == pytest.approx(0.03, rel=1e-3)
    assert grad_report([("to_k.bias", -r, r)], COS_MIN, GREL_MAX)[2]


def test_the_old_gradient_loop_accepted_nan():
    """why `if cos < a or rel > b: bad.append(..)` and `worst = max(worst, rel)` are gone: both comparisons are False for NaN and max()
    keeps the old value"""
    ref, got = _grads()
    m = dict(got); m["b.weight"] = torch.full_like(got["b.weight"], float("nan"))
    worst, bad = old_grad_loop([(n, m[n].double(), ref[n]) for n in ref], COS_MIN, GREL_MAX)
    assert not bad and worst < 2.0 ** -8                         # a gradient that is entirely NaN: reported as fine, and the print hid it
    m = dict(got); m["a.weight"] = -got["a.weight"]
    assert old_grad_loop([(n, m[n].double(), ref[n]) for n in ref], COS_MIN, GREL_MAX)[1]    # it did see finite errors


# ------------------------------------------------------------------ bars from the bf16 noise floor
def test_grad_report_takes_a_bar_per_parameter_and_a_missing_name_is_an_error():
    ref, got = _grads()
    pairs = [(n, got[n], ref[n]) for n in ref]
    bars = {n: GREL_MAX for n in ref}
    assert grad_report(pairs, COS_MIN, bars) == grad_report(pairs, COS_MIN, GREL_MAX)              # a float keeps its behaviour
    m = dict(got); m["a.weight"] = got["a.weight"] * 1.03; m["b.weight"] = got["b.weight"] * 1.03
    bars["a.weight"] = 0.02
    _, _, bad = grad_report([(n, m[n], ref[n]) for n in ref], COS_MIN, bars)
    assert [b[0] for b in bad] == ["a.weight"]                    # 3 % off: over its own 2 % bar, b.weight under the flat 15 %
    del bars["norm.weight"]
    with pytest.raises(KeyError, match=r"norm\.weight: no rel-L2 bar"):
        grad_report(pairs, COS_MIN, bars)
    with pytest.raises(KeyError):
        grad_report(pairs, COS_MIN, {})


def test_grad_floor_measures_the_bf16_restatement_and_refuses_non_finite_entries():
    ref, got = _grads()
    floor, overall = grad_floor(got, ref)
    assert set(floor) == set(ref) and all(0 < f < 2.0 ** -8 for f in floor.values())
    assert floor["a.bias"] == pytest.approx(rel_l2(got["a.bias"], ref["a.bias"]))
    tot = sum((got[n].double() - ref[n]).pow(2).sum() for n in ref).sqrt() / sum(ref[n].pow(2).sum() for n in ref).sqrt()
    assert overall == pytest.approx(tot.item())
    for side in ("noisy", "ref"):
        for val in (float("nan"), float("inf")):
            a, b = dict(got), dict(ref)
            d = a if side == "noisy" else b
            t = d["b.weight"].clone(); t[3, 3] = val; d["b.weight"] = t
            with pytest.raises(ValueError, match=r"b\.weight"):
                grad_floor(a, b)
    with pytest.raises(KeyError):
        grad_floor({n: got[n] for n in list(got)[:-1]}, ref)
    m = dict(got); m["a.bias"] = None
    with pytest.raises(ValueError, match=r"a\.bias"):
        grad_floor(m, ref)


def test_floor_bars_cap_at_the_old_bar_clamp_at_the_median_and_limit_exceptions():
    floor = {"lucky": 1e-4, "low": 0.01, "mid": 0.02, "high": 0.04, "noisy": 0.3}
    bars = floor_bars(floor, 0.2)
    assert parity.MARGIN == 1.5
    assert bars == {"lucky": pytest.approx(0.03), "low": pytest.approx(0.03), "mid": pytest.approx(0.03), "high": pytest.approx(0.06), "noisy": 0.2}
    assert all(b <= 0.2 for b in floor_bars(floor, 0.2, margin=100.0).values())           # whatever the margin, no bar above the old one
    assert overall_bar(5e-2, 0.02) == pytest.approx(0.03) and overall_bar(5e-2, 0.2) == 5e-2
    # an exception: a cause in words, a margin of at most 3, at most 1 % of the parameters, never above the old bar
    many = {f"p{i}": 0.02 for i in range(200)}
    ex = floor_bars(many, 0.2, exceptions={"p7": (3.0, "fp32-atomic dQ hand-off the restatement does not have")})
    assert ex["p7"] == pytest.approx(0.06) and ex["p8"] == pytest.approx(0.03)
    assert floor_bars(many, 0.05, exceptions={"p7": (3.0, "cause")})["p7"] == 0.05
    for bad in ({"p7": (3.5, "cause")}, {"p7": (2.0, " ")}, {"nope": (2.0, "cause")}, {f"p{i}": (2.0, "cause") for i in range(3)}):
        with pytest.raises(AssertionError):
            floor_bars(many, 0.2, exceptions=bad)
    with pytest.raises(AssertionError):
        floor_bars(floor, 0.2, exceptions={"high": (2.0, "one of five parameters is more than 1 %")})


def test_floor_report_flags_what_the_flat_bar_let_through():
    """a gradient 5 % off passes the flat 15 % bar and fails a bar derived from a 0.2 % floor; the report names the worst ratio"""
    ref, got = _grads()
    m = {n: g.double() for n, g in got.items()}
    m["b.weight"] = ref["b.weight"] * 1.05
    pairs = [(n, m[n], ref[n]) for n in ref]
    assert not grad_report(pairs, COS_MIN, GREL_MAX)[2]
    overall, ofloor, worst, bad, ratio, at = floor_report(pairs, got, COS_MIN, GREL_MAX)
    assert [b[0] for b in bad] == ["b.weight"] and at == "b.weight" and worst == pytest.approx(0.05)
    assert 0 < ofloor < 2.0 ** -8 and ratio > 10
    o2, f2, w2, bad2, r2, _ = floor_report([(n, got[n], ref[n]) for n in ref], got, COS_MIN, GREL_MAX)          # the restatement against its own floor
    assert not bad2 and o2 == pytest.approx(f2) and r2 <= 1.0 + 1e-12
    with pytest.raises(KeyError):
        floor_report(pairs, {n: got[n] for n in list(got)[:2]}, COS_MIN, GREL_MAX)


# ------------------------------------------------------------------ poisoned / untouched
DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64,
          torch.float8_e4m3fn, torch.float8_e5m2]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_poison_round_trips_bit_exactly_and_untouched_sees_one_element(dtype):
    buf = poisoned((5, 24), dtype, "cpu")
    assert buf.dtype == dtype and buf.shape == (5, 24) and bool(is_poison(buf).all())
    assert bool(is_poison(buf.clone()).all()) and bool(is_poison(poisoned_like(buf)).all())
    if dtype in (torch.float32, BF, torch.float16, torch.float64):
        assert bool(torch.isnan(buf).all())
    if dtype == BF:
        assert bool((buf.view(torch.int16) == parity.SENT).all())
    if buf.element_size() == 1:
        assert bool((buf.view(torch.uint8) == parity.SENT8).all())
    one = torch.ones((), dtype=torch.float32).to(dtype)
    region = (slice(1, 4), slice(0, 16))
    untouched(buf, region, "nothing written")
    untouched(buf, [], "nothing written, empty region")
    with pytest.raises(AssertionError, match="never written"):
        all_written(buf[region], "region")
    buf[1:4, :16] = one                                          # inside the region: not a finding
    untouched(buf, region, "region written")
    untouched(buf, [(slice(1, 2),), (slice(2, 4), slice(0, 16))], "region as a list of pieces; the first covers more")
    all_written(buf[region], "region")
    mask = torch.zeros(5, 24, dtype=torch.bool); mask[region] = True
    untouched(buf, mask, "region as a mask")
    for where in ((0, 0), (3, 16), (4, 23), (1, 23)):            # outside: one element is enough
        b2 = buf.clone(); b2[where] = one
        with pytest.raises(AssertionError, match="1 elements outside"):
            untouched(b2, region, "one element")
        with pytest.raises(AssertionError, match="1 elements outside"):
            untouched(b2, mask, "one element")
    b2 = buf.clone(); b2[2, 3] = poisoned((), dtype, "cpu")      # an element of the region left as it was
    with pytest.raises(AssertionError, match="1 of 48 elements were never written"):
        all_written(b2[region], "hole")


@pytest.mark.parametrize("dtype", [torch.float32, BF, torch.float16, torch.float64], ids=lambda d: str(d).split(".")[-1])
def test_a_nan_the_kernel_wrote_is_not_the_poison(dtype):
    """the poison of every float type is a NaN with a payload of its own: a NaN a kernel computes (the default quiet NaN, here 0 / 0 and
    inf - inf in that type) and stores in the guard region is seen as a write"""
    buf = poisoned((8,), dtype, "cpu")
    assert bool(torch.isnan(buf).all())
    zero, inf = torch.zeros((), dtype=dtype), torch.full((), float("inf"), dtype=dtype)
    buf[3] = zero / zero
    buf[6] = inf - inf
    with pytest.raises(AssertionError, match="2 elements outside"):
        untouched(buf, [], "computed NaN")


def test_all_written_allows_the_sentinel_byte_where_the_expected_result_holds_it():
    """0x5A is 20.0 in e4m3: a correct output may hold it, but only where the bit-exact expected result does"""
    F8 = torch.float8_e4m3fn
    want = torch.tensor([1.0, 20.0, -3.0, 20.0]).to(F8)
    got = want.clone()
    all_written(got, "exact", expect=want)
    with pytest.raises(AssertionError, match="2 of 4"):
        all_written(got, "without the expected result")
    got = poisoned((4,), F8, "cpu"); got[1] = want[1]; got[3] = want[3]; got[0] = want[0]
    with pytest.raises(AssertionError, match="1 of 4 elements were never written .first at flat index 2"):
        all_written(got, "hole", expect=want)
    with pytest.raises(TypeError):
        poisoned((4,), torch.bool, "cpu")


# ------------------------------------------------------------------ the GPU test sources
GPU_SOURCES = sorted(glob.glob(os.path.join(HERE, "*_gpu.py"))) + [os.path.join(HERE, "grad_clip_common.py")]
FORBIDDEN_DEFS = {"close", "_rel", "_relerr", "relerr", "_grad_report", "_check_param_grads",
                  # the floor-derived bars have one home too: a GPU test builds no bars, floors or margins of its own
                  "grad_report", "grad_floor", "floor_bars", "floor_report", "_floor_report", "floor_ratio", "overall_bar", "MARGIN"}
EMPTY = re.compile(r"\b(new_)?empty(_like|_strided)?\s*\(")
# every torch.empty / empty_like left in a GPU test: (file, the stripped line, why it is not a kernel output).  A buffer that a kernel
# writes whole does not belong here: it is allocated with parity.poisoned.
EMPTY_ALLOWED = [
    ("test_fullsize_gpu.py", "o = torch.empty_like(q); lse = torch.empty(S)", "host tensors of the chunked fp32 CPU reference, filled chunk by chunk by torch"),
    ("test_fullsize_gpu.py", "dq = torch.empty_like(q); dk = torch.zeros_like(k); dv = torch.zeros_like(v)", "host tensor of the same CPU reference"),
]


def test_gpu_tests_define_no_comparator_of_their_own():
    assert len(GPU_SOURCES) > 15
    found = []
    for path in GPU_SOURCES:
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)) and node.name in FORBIDDEN_DEFS:
                found.append(f"{os.path.basename(path)}:{node.lineno} defines {node.name}")
            if isinstance(node, ast.Assign):
                for t in node.targets:
                    if isinstance(t, ast.Name) and t.id in FORBIDDEN_DEFS:
                        found.append(f"{os.path.basename(path)}:{node.lineno} assigns {t.id}")
    assert not found, "comparators belong to tests/parity.py: " + "; ".join(found)


def test_gpu_tests_allocate_no_output_with_torch_empty():
    allowed = {(f, line) for f, line, why in EMPTY_ALLOWED}
    assert all(why.strip() for _, _, why in EMPTY_ALLOWED)
    seen, extra = set(), []
    for path in GPU_SOURCES:
        name = os.path.basename(path)
        for no, line in enumerate(open(path), 1):
            code = line.split("#", 1)[0]
            if EMPTY.search(code) and "empty_cache" not in code:
                key = (name, line.strip())
                if key in allowed:
                    seen.add(key)
                else:
                    extra.append(f"{name}:{no}: {line.strip()}")
    assert not extra, "allocate kernel outputs with parity.poisoned (or list the line in EMPTY_ALLOWED with its reason): " + "; ".join(extra)
    assert seen == allowed, f"EMPTY_ALLOWED lists lines that are gone: {sorted(allowed - seen)}"


# the NaN-blind per-parameter idiom: `worst = max(worst, rel)` keeps the old value when rel is NaN, and a hand-made `x.norm().item() / ...`
# ratio is where such a rel comes from.  Every line of a GPU test that still has one of the two shapes is listed with why it is safe.
BLIND = re.compile(r"\bmax\(\s*worst\s*,|\.norm\(\)\.item\(\)\s*/")
BLIND_ALLOWED = [
    ("test_gemm_production_gpu.py", "worst = max(worst, loss / 2.0 ** 16)", "`assert loss <= limit` on the line before fails for a NaN loss"),
    ("test_hunyuan_sp_gpu.py", "worst = max(worst, rel_l2(a, b))", "parity.rel_l2 refuses non-finite input"),
    ("test_hunyuan_mxfp8_gpu.py", "f\"|contribution| / |out| {res['weights'][0].norm().item() / res['weights'][2].norm().item():.3e}; out mfma vs weights \"",
     "a ratio inside a printed line; the assertion after it compares the two norms without dividing"),
]


def test_gpu_tests_have_no_nan_blind_worst_loop():
    allowed = {(f, line) for f, line, _ in BLIND_ALLOWED}
    extra = []
    for path in GPU_SOURCES:
        name = os.path.basename(path)
        for no, line in enumerate(open(path), 1):
            if BLIND.search(line) and (name, line.strip()) not in allowed:
                extra.append(f"{name}:{no}: {line.strip()}")
    assert not extra, "use parity.rel_l2 / parity.grad_report (they refuse non-finite gradients): " + "; ".join(extra)


def test_the_source_checks_see_a_reintroduced_comparator_and_an_unlisted_empty(tmp_path, monkeypatch):
    src = ("import torch\n\n\ndef close(a, b, rtol, atol, what=''):\n    assert ((a - b).abs() > atol).float().mean() == 0\n\n\n"
           "def test_x(dev):\n    out = torch.empty(4, 4, device=dev)\n    cache = torch.cuda.empty_cache()\n")
    p = tmp_path / "test_new_gpu.py"
    p.write_text(src)
    monkeypatch.setattr(__import__(__name__), "GPU_SOURCES", GPU_SOURCES + [str(p)])
    with pytest.raises(AssertionError, match="test_new_gpu.py:4 defines close"):
        test_gpu_tests_define_no_comparator_of_their_own()
    with pytest.raises(AssertionError, match=r"test_new_gpu.py:9: out = torch.empty\(4, 4, device=dev\)"):
        test_gpu_tests_allocate_no_output_with_torch_empty()
    p.write_text("def test_y(dev):\n    worst = 0.0\n    for gd, gr in pairs:\n        rel = (gd - gr).norm().item() / max(gr.norm().item(), 1e-12)\n"
                 "        worst = max(worst, rel)\n    assert worst < 6e-2\n")
    with pytest.raises(AssertionError, match=r"test_new_gpu.py:4: rel = .*; test_new_gpu.py:5: worst = max\(worst, rel\)"):
        test_gpu_tests_have_no_nan_blind_worst_loop()
