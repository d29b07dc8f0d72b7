"""The comparison and output-buffer helpers every GPU parity test shares.

Three rules, each closing a way a wrong kernel used to pass:
  * a comparison accepts an element only when `err <= tol` holds, so NaN and Inf on the device side are out of tolerance
    (`err > tol` is False for NaN; the old `(err > tol).float().mean()` let an all-NaN output through);
  * per-parameter gradient reports accept a parameter only when `cos > cos_min and rel < rel_max` holds, the worst figure
    propagates NaN, and every device gradient must be finite;
  * an output a kernel writes whole is allocated with `poisoned`, never `torch.empty`: the caching allocator hands a just
    freed block of the same size to the next variant of a test, and "empty" memory then already holds a correct result.
    What lies outside a kernel's contract region is checked bit for bit with `untouched`.
A non-finite REFERENCE is a bug of the test and raises ValueError."""
import math

import torch

SENT = 0x7FA5             # poison bf16 bits: a NaN whose payload no kernel produces
SENT8 = 0x5A              # poison byte of 1-byte types (uint8 / int8 / fp8) and of every other non-float type
# the poison of every float type is a NaN with a payload of its own (set through the integer view), so that a NaN a kernel COMPUTES and
# stores outside its region (the default quiet NaN) is told from the poison by `untouched`
_NAN_BITS = {torch.bfloat16: (torch.int16, SENT), torch.float16: (torch.int16, 0x7DA5), torch.float32: (torch.int32, 0x7FA5A5A5),
             torch.float64: (torch.int64, 0x7FF5A5A5A5A5A5A5)}
_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _ref64(ref, what):
    ref = ref.detach().double().cpu()
    if not bool(torch.isfinite(ref).all()):
        raise ValueError(f"{what}: the reference holds {int((~torch.isfinite(ref)).sum())} non-finite elements (a bug of the test)")
    return ref


def close(got, ref, rtol, atol, what=""):
    """every element of got within atol + rtol * |ref| of ref; NaN / Inf in got are out of tolerance"""
    got = got.detach().double().cpu()
    ref = _ref64(ref, what)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against the reference's {tuple(ref.shape)}"
    if got.numel() == 0:
        return
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    ok = err <= tol                                            # False for NaN and Inf
    if bool(ok.all()):
        return
    nonfinite = int((~torch.isfinite(got)).sum())
    excess = torch.where(ok, torch.full_like(err, -1.0), torch.nan_to_num(err - tol, nan=math.inf, posinf=math.inf))
    at = int(excess.flatten().argmax())
    finite_err = err[torch.isfinite(err)]
    mx = finite_err.max().item() if finite_err.numel() else float("nan")
    raise AssertionError(f"{what}: {(~ok).double().mean().item() * 100:.4f}% out of tol, max err {mx:.4g}, ref absmax {ref.abs().max().item():.4g}, "
                         f"worst at flat index {at} (got {got.flatten()[at].item():.6g}, ref {ref.flatten()[at].item():.6g}), "
                         f"{nonfinite} non-finite elements")


def _finite64(t, what):
    t = t.detach().double().cpu()
    assert bool(torch.isfinite(t).all()), f"{what}: {int((~torch.isfinite(t)).sum())} non-finite elements of {t.numel()}"
    return t


def rel_l2(got, ref):
    """|got - ref| / |ref| in fp64; both sides must be finite"""
    a = _finite64(got, "rel_l2: got")
    b = _ref64(ref, "rel_l2: ref")
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def relerr(got, ref):
    """(rel-L2, max error over the reference's absmax); both sides must be finite"""
    a = _finite64(got, "relerr: got")
    b = _ref64(ref, "relerr: ref")
    return ((a - b).norm() / b.norm()).item(), ((a - b).abs().max() / b.abs().max()).item()


def cosine(got, ref):
    a = _finite64(got, "cosine: got").flatten()
    b = _ref64(ref, "cosine: ref").flatten()
    return (a @ b / (a.norm() * b.norm()).clamp_min(1e-300)).item()


def grad_report(pairs, cos_min, rel_max):
    """pairs: (name, device gradient, reference gradient).  Returns (overall rel-L2, worst per-parameter rel-L2, bad) where bad lists
    (name, rel, cos) of every parameter that is not `cos > cos_min and rel < rel_max`; a NaN figure is bad and makes worst NaN.
    rel_max: one float for every parameter, or a mapping name -> bar (see `floor_bars`); a name the mapping does not hold is an error.
    Every device gradient must be finite: the first that is not fails the report by name."""
    worst, bad, tot_n, tot_d = 0.0, [], 0.0, 0.0
    n_pairs = 0
    per_name = not isinstance(rel_max, (int, float))
    for name, gd, gr in pairs:
        n_pairs += 1
        assert gd is not None, f"{name}: no device gradient"
        if per_name and name not in rel_max:
            raise KeyError(f"{name}: no rel-L2 bar for this parameter (a parameter without a bar is not a pass)")
        bar = rel_max[name] if per_name else rel_max
        gd = gd.detach().double().cpu().flatten()
        gr = _ref64(gr, f"{name}: reference gradient").flatten()
        assert gd.shape == gr.shape, f"{name}: gradient of {gd.numel()} elements against the reference's {gr.numel()}"
        assert bool(torch.isfinite(gd).all()), f"{name}: {int((~torch.isfinite(gd)).sum())} non-finite gradient elements of {gd.numel()}"
        e = (gd - gr).norm().item(); d = gr.norm().item()
        tot_n += e * e; tot_d += d * d
        rel = e / max(d, 1e-12)
        cos = torch.nn.functional.cosine_similarity(gd, gr, dim=0).item()      # each norm clamped at 1e-8 on its own: tiny gradients keep their angle
        if not (cos > cos_min and rel < bar):
            bad.append((name, rel, cos))
        worst = float("nan") if math.isnan(rel) or math.isnan(worst) else max(worst, rel)
    assert n_pairs > 0, "grad_report: no gradients to compare"
    overall = math.sqrt(tot_n) / max(math.sqrt(tot_d), 1e-30)
    return overall, worst, bad


# ------------------------------------------------------------------ bars from the reference's own bf16 noise floor
# The fp64 oracle restated in bf16 on the CPU (same bf16-rounded weights, inputs, masks and upstream gradient; every op rounds its result
# to bf16) is one sample of the rounding noise a correct bf16 implementation carries.  The device keeps fp32 accumulators and rounds at
# stores only, so its own sample is expected to be the smaller one; MARGIN covers the parameter-to-parameter scatter between two draws.
MARGIN = 1.5
EXCEPTION_MARGIN_MAX = 3.0          # a parameter behind a rounding point only the device has (stated with its cause where it is used)
EXCEPTION_SHARE_MAX = 0.01          # at most this share of a model's parameters


def _median(values):
    v = sorted(values)
    assert v, "median of nothing"
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def grad_floor(noisy, ref):
    """noisy, ref: {name: gradient} of the bf16 and of the fp64 restatement of the same model.  Returns ({name: rel-L2}, overall rel-L2
    over all parameters).  Both must hold the same names; a non-finite entry on either side raises ValueError (a bug of the test)."""
    if set(noisy) != set(ref):
        raise KeyError(f"grad_floor: the two runs hold different parameters: {sorted(set(noisy) ^ set(ref))[:6]}")
    assert ref, "grad_floor: no gradients"
    floor, tot_n, tot_d = {}, 0.0, 0.0
    for name, r in ref.items():
        if noisy[name] is None or r is None:
            raise ValueError(f"{name}: a restatement left no gradient (a bug of the test)")
        a = _ref64(noisy[name], f"{name}: bf16 restatement").flatten()
        b = _ref64(r, f"{name}: fp64 restatement").flatten()
        if a.shape != b.shape:
            raise ValueError(f"{name}: {a.numel()} elements in the bf16 restatement, {b.numel()} in the fp64 one")
        e = (a - b).norm().item(); d = b.norm().item()
        tot_n += e * e; tot_d += d * d
        floor[name] = e / max(d, 1e-12)
    return floor, math.sqrt(tot_n) / max(math.sqrt(tot_d), 1e-30)


def _clamped(floor):
    med = _median(floor.values())
    return {n: max(f, med) for n, f in floor.items()}


def floor_bars(floor, rel_max, margin=MARGIN, exceptions=None):
    """{name: min(rel_max, margin * max(floor[name], median floor))}: the old flat bar stays as the cap, and a parameter whose bf16 draw
    happened to land unusually close to fp64 is held to the model's median, a bar an independent noise sample can meet.
    exceptions: {name: (margin, cause)} for a parameter behind a rounding point that only the device has -- margin at most 3, at most 1 %
    of the model's parameters, a cause in words, and still never above rel_max."""
    assert floor and rel_max > 0 and margin > 0
    exceptions = exceptions or {}
    assert set(exceptions) <= set(floor), f"exceptions for parameters the model does not have: {sorted(set(exceptions) - set(floor))}"
    assert len(exceptions) <= EXCEPTION_SHARE_MAX * len(floor), f"{len(exceptions)} exceptions for {len(floor)} parameters"
    for n, (mg, cause) in exceptions.items():
        assert margin <= mg <= EXCEPTION_MARGIN_MAX and str(cause).strip(), f"{n}: exception margin {mg} / cause {cause!r}"
    return {n: min(rel_max, (exceptions[n][0] if n in exceptions else margin) * f) for n, f in _clamped(floor).items()}


def overall_bar(rel_max, overall_floor, margin=MARGIN):
    """the bar of the overall rel-L2: the old one, or margin x the bf16 restatement's own overall figure where that is lower"""
    return min(rel_max, margin * overall_floor)


def floor_ratio(pairs, floor):
    """(worst rel-L2 / clamped floor over the parameters, the parameter that has it): what a test prints next to its other figures"""
    cl, worst, at = _clamped(floor), -1.0, None
    for name, gd, gr in pairs:
        r = rel_l2(gd, gr) / max(cl[name], 1e-30)
        if at is None or not (r <= worst):
            worst, at = r, name
    assert at is not None, "floor_ratio: no gradients"
    return worst, at


def floor_report(pairs, noisy, cos_min, rel_max, exceptions=None):
    """grad_report with floor-derived bars.  pairs: a list of (name, device gradient, fp64 reference gradient); noisy: {name: gradient of the
    same step restated in bf16 on the CPU}; rel_max: the old flat bar, kept as the cap.  Returns (overall rel-L2, overall bf16 floor, worst
    per-parameter rel-L2, bad, worst device / floor ratio, the parameter that has it)"""
    pairs = list(pairs)
    floor, ofloor = grad_floor({n: noisy[n] for n, _, _ in pairs}, {n: r for n, _, r in pairs})
    overall, worst, bad = grad_report(pairs, cos_min, floor_bars(floor, rel_max, exceptions=exceptions))
    return (overall, ofloor, worst, bad) + floor_ratio(pairs, floor)


def bf16_leaves(params):
    """{name: a bf16 leaf that requires grad} of the tensors in params (other entries, such as a LoRA scaling float, pass through)"""
    return {k: (v.detach().to(torch.bfloat16).requires_grad_(True) if isinstance(v, torch.Tensor) else v) for k, v in params.items()}


# ------------------------------------------------------------------ poisoned outputs
def _fill_poison(t):
    if t.dtype == torch.bool:
        raise TypeError("poisoned: bool has no value a kernel cannot produce; use uint8")
    if t.numel() == 0:
        return t
    if t.dtype in _NAN_BITS:
        as_int, bits = _NAN_BITS[t.dtype]
        t.view(-1).view(as_int).fill_(bits)
    else:
        t.view(-1).view(torch.uint8).fill_(SENT8)
    return t


def poisoned(shape, dtype, device):
    """an output buffer of `shape` (a tuple) no correct kernel leaves as it is: a NaN with a payload of its own for fp32 / bf16 / fp16 /
    fp64, the SENT8 byte pattern for integer and fp8 types"""
    return _fill_poison(torch.empty(tuple(shape), dtype=dtype, device=device))


def poisoned_like(t, dtype=None):
    """a contiguous poisoned buffer of t's shape, dtype (unless given) and device"""
    return poisoned(tuple(t.shape), dtype or t.dtype, t.device)


def _bits(t):
    t = t.detach().contiguous()
    return t.view(_BITS[t.element_size()])


def is_poison(t):
    """elementwise: does the element still hold the poison bits"""
    ref = _fill_poison(torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device))
    b, r = _bits(t), _bits(ref)
    return (b == r).view(t.shape) if b.numel() else torch.zeros(t.shape, dtype=torch.bool, device=t.device)


def all_written(t, what="", expect=None):
    """no element of the contract region still holds the poison bits (stated for sentinel-typed outputs, where a comparison against a
    reference does not imply it by itself).  The SENT8 byte is a legal value of the 1-byte types (20.0 in e4m3): with `expect`, the
    bit-exact expected result of the same dtype, an element may hold the poison bits only where the expected result holds them too."""
    left = is_poison(t)
    if expect is not None:
        assert expect.dtype == t.dtype and expect.shape == t.shape, f"{what}: expect must have the output's dtype and shape"
        left &= ~is_poison(expect).to(t.device)
    n = int(left.sum())
    assert n == 0, f"{what}: {n} of {t.numel()} elements were never written (first at flat index {int(left.flatten().int().argmax())})"


def untouched(buf, region, what=""):
    """the poison of `buf` (allocated with `poisoned`) outside `region` is still there bit for bit.  region: a bool mask of buf's shape
    (True = the kernel's contract region), an index / slice / tuple of them as in buf[region], or a list of such tuples."""
    if isinstance(region, torch.Tensor) and region.dtype == torch.bool:
        inside = region.to(buf.device)
        assert inside.shape == buf.shape, f"{what}: mask of shape {tuple(inside.shape)} for a buffer of {tuple(buf.shape)}"
    else:
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
        for r in (region if isinstance(region, list) else [region]):
            inside[r] = True
    hit = ~is_poison(buf) & ~inside
    n = int(hit.sum())
    assert n == 0, f"{what}: {n} elements outside the output region were written (first at flat index {int(hit.flatten().int().argmax())})"
