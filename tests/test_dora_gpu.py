"""DoRA adapters (LoraConfig.use_dora) on the GPU: the kernels of csrc/dora.hip through vt355.ops -- the row norms, the scaled operand
refresh -- and the training step through the module interface against the fp64 restatement of tests/dora_ref.py.

Kernel shapes follow the sibling tests: N = 200 rows (one full 32-row block group and a partial one; three 64-row transpose tiles and 8
rows), K = 192 (three 64-column tiles; 24 of a wave's 64 lanes hold a chunk), padded leading dimensions, sentinel rows around and
poisoned (tests/parity.py) outputs."""
import pytest
import torch

import dora_ref as R
from parity import poisoned, rel_l2, untouched

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N0, K0 = 200, 192
ATTN = list(R.TARGETS[:4])
SIX = list(R.TARGETS)
# fp32 against fp64 of the plain torch evaluation norm(W + s B @ A) on the CPU over the ten (r, n) cases below: worst relative error
# 1.46e-7 (1.454e-7 rounded up).  The device's sum is another draw of the same rounding: it gets twice that.
NORM_CPU_FP32_ERR = 1.46e-7
NORM_BAR = 2 * NORM_CPU_FP32_ERR


def rb(x):
    return x.to(BF).float()


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def sparse_ints(g, lo, hi, keep_one_in, *shape):
    return ints(g, lo, hi, *shape) * (torch.randint(0, keep_one_in, shape, generator=g) == 0).double()


def ref_sumsq(W, A, B, n, r, s):
    """fp64 sum of squares of the rows of W + s B A, adapter j on its own row block"""
    N = W.shape[0] // n
    return torch.cat([((W[j * N:(j + 1) * N] + s * B[j * N:(j + 1) * N] @ A[j * r:(j + 1) * r]) ** 2).sum(1) for j in range(n)])


def launch_norm(dev, W, A, B, n, r, s, mag=None, ldw_pad=40, lda_pad=8):
    """W / A in padded buffers (NaN in the padding), B contiguous at an odd element offset of its buffer (the flat bf16 copy gives it no more
    than 2-byte alignment), the output poisoned with sentinel elements around"""
    from vt355 import ops
    Nn, K = W.shape
    wb = torch.full((Nn, K + ldw_pad), float("nan"), dtype=BF, device=dev); wb[:, :K] = W.to(dev, BF)
    ab = torch.full((A.shape[0], K + lda_pad), float("nan"), dtype=BF, device=dev); ab[:, :K] = A.to(dev, BF)
    bb = torch.zeros(Nn * r + 1, dtype=BF, device=dev); bv = bb[1:].view(Nn, r); bv.copy_(B.to(dev, BF))
    out = poisoned((Nn + 16,), torch.float32, dev)
    ops.dora_norm(wb[:, :K], ab[:, :K], bv, n, r, s, out[8:8 + Nn], mag=None if mag is None else mag.to(dev))
    torch.cuda.synchronize()
    region = torch.zeros(Nn + 16, dtype=torch.bool); region[8:8 + Nn] = True
    untouched(out, region, "dora_norm wrote outside its rows")
    return out[8:8 + Nn].cpu()


# ================================================================== the norm kernel
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("r", [4, 16, 20, 40, 128])
def test_norm_exact_on_small_integers(dev, r, n):
    """W in [-3, 3], A and B in {-1, 0, 1} (one in four / one in two non-zero), s = 2: every element of W + s B A and every partial sum of
    squares is an integer below 2^24 (asserted on the fp64 reference), so fp32 holds the sum exactly whatever the order, and the result is
    the fp32 square root of that integer to 1 ulp"""
    g = torch.Generator().manual_seed(100 + r + n)
    W, A, B = ints(g, -3, 3, n * N0, K0), sparse_ints(g, -1, 1, 4, n * r, K0), sparse_ints(g, -1, 1, 2, n * N0, r)
    ss = ref_sumsq(W, A, B, n, r, 2.0)
    assert 0 < ss.min().item() and ss.max().item() < 2 ** 24 and torch.equal(ss, ss.round())
    want = torch.sqrt(ss.float())
    got = launch_norm(dev, W, A, B, n, r, 2.0)
    lo, hi = torch.nextafter(want, torch.zeros_like(want)), torch.nextafter(want, torch.full_like(want, float("inf")))
    bad = (got < lo) | (got > hi) | torch.isnan(got)
    assert not bad.any(), f"{int(bad.sum())} of {got.numel()} norms are more than 1 ulp off"
    assert not torch.equal(ss, (W ** 2).sum(1)), "the adapters do not reach the norm"
    if n == 3:          # every adapter read its own rows of A and B
        for j in range(3):
            other = ref_sumsq(W[j * N0:(j + 1) * N0], A[(j + 1) % 3 * r:((j + 1) % 3 + 1) * r], B[j * N0:(j + 1) * N0], 1, r, 2.0)
            assert not torch.equal(other, ss[j * N0:(j + 1) * N0])


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("r", [4, 16, 20, 40, 128])
def test_norm_randn_against_fp64(dev, r, n):
    """randn operands (bf16-rounded, W ~ 0.02, A ~ 0.09, B ~ 0.05, s = 0.7) against fp64.  The bar is not a guess: torch's own fp32
    evaluation of norm(W + s B @ A) on the CPU is within 1.46e-7 (relative, worst of these ten cases: 1.454e-7) of fp64; the device's fp32 sum is
    another draw of the same rounding and gets twice that, 2.92e-7.  c = m / norm (the mag form) adds one correctly rounded division:
    half an ulp, 6e-8."""
    g = torch.Generator().manual_seed(900 + r + n)
    W, A, B = rb(torch.randn(n * N0, K0, generator=g) * 0.02), rb(torch.randn(n * r, K0, generator=g) * 0.09), rb(torch.randn(n * N0, r, generator=g) * 0.05)
    ref = ref_sumsq(W.double(), A.double(), B.double(), n, r, 0.7).sqrt()
    cpu32 = torch.cat([torch.linalg.norm(W[j * N0:(j + 1) * N0] + 0.7 * (B[j * N0:(j + 1) * N0] @ A[j * r:(j + 1) * r]), dim=1) for j in range(n)])
    got = launch_norm(dev, W, A, B, n, r, 0.7)
    e_cpu, e_dev = ((cpu32.double() - ref).abs() / ref).max().item(), ((got.double() - ref).abs() / ref).max().item()
    print(f"r={r} n={n}: worst relative error of the norm: CPU fp32 {e_cpu:.3e}, device {e_dev:.3e} (bar {NORM_BAR:.3e})")
    assert e_dev <= NORM_BAR
    m = torch.rand(n * N0, generator=g) + 0.5
    c = launch_norm(dev, W, A, B, n, r, 0.7, mag=m)
    e_c = ((c.double() - m.double() / ref).abs() / (m.double() / ref)).max().item()
    assert e_c <= NORM_BAR + 6e-8, e_c


def test_norm_at_k7680(dev):
    """K = 7680 = 4 x 1920, ff.net.2's in_features at 2B: 960 chunks, 15 per lane.  Exact integers as above (W in [-1, 1], r = 20)"""
    g = torch.Generator().manual_seed(7680)
    Nn, K, r = 64, 7680, 20
    W, A, B = ints(g, -1, 1, Nn, K), sparse_ints(g, -1, 1, 4, r, K), sparse_ints(g, -1, 1, 2, Nn, r)
    ss = ref_sumsq(W, A, B, 1, r, 2.0)
    assert ss.max().item() < 2 ** 24
    want = torch.sqrt(ss.float())
    got = launch_norm(dev, W, A, B, 1, r, 2.0)
    assert ((got >= torch.nextafter(want, torch.zeros_like(want))) & (got <= torch.nextafter(want, torch.full_like(want, float("inf"))))).all()


def test_same_operands_give_the_same_bits_and_c_is_one(dev):
    """m initialised from the kernel makes c == 1.0f exactly: the sum's order depends on the shape only"""
    g = torch.Generator().manual_seed(5)
    W, A, B = rb(torch.randn(N0, K0, generator=g) * 0.02), rb(torch.randn(20, K0, generator=g) * 0.09), torch.zeros(N0, 20)
    m = launch_norm(dev, W, A, B, 1, 20, 0.25)
    assert torch.equal(m, launch_norm(dev, W, A, B, 1, 20, 0.25))
    assert torch.equal(launch_norm(dev, W, A, B, 1, 20, 0.25, mag=m), torch.ones(N0))


# ================================================================== the refresh kernels
def _frame(dev, rows, cols, pad):
    """a poisoned [rows + 2, cols + pad] buffer and its [rows, cols] body"""
    buf = poisoned((rows + 2, cols + pad), BF, dev)
    return buf, buf[1:rows + 1, :cols]


def _expect(w, c, by_col=False):
    return ((c[None, :] if by_col else c[:, None]) * w.float()).to(BF)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


@pytest.mark.parametrize("by_col", [False, True], ids=["by_row", "by_col"])
def test_scale_from_the_pristine_weight_is_one_rounding(dev, by_col):
    """dst = bf16(c * w) bit for bit against torch's (c * w.float()).to(bf16), randn c and W, both factor orientations; the source (padded
    leading dimension) and everything around the destination stay as they were"""
    from vt355 import ops
    g = torch.Generator().manual_seed(11 + by_col)
    w = (torch.randn(N0, K0, generator=g) * 0.02).to(BF)
    c = torch.randn(K0 if by_col else N0, generator=g)
    src = torch.full((N0, K0 + 24), float("nan"), dtype=BF, device=dev); src[:, :K0] = w.to(dev)
    before = src.clone()
    buf, dst = _frame(dev, N0, K0, 72)
    ops.dora_scale(src[:, :K0], dst, c.to(dev), by_col=by_col)
    torch.cuda.synchronize()
    assert _same_bits(dst.cpu(), _expect(w, c, by_col))
    assert _same_bits(src.cpu(), before.cpu())
    untouched(buf, (slice(1, N0 + 1), slice(0, K0)), "dora_scale wrote outside the operand")


@pytest.mark.parametrize("r,rp,ext", [(4, 4, 64), (16, 16, 64), (20, 32, 64), (40, 48, 64), (128, 128, 128)], ids=["r4", "r16", "r20", "r40", "r128"])
def test_extension_parts_scale_in_place_and_zero_columns_stay_zero(dev, r, rp, ext):
    """the extension columns [c s B | 0] of a forward operand (factor per row) and the s B^T extension rows of a transposed one (factor per
    column), in place behind a base part that must not change: narrow (r <= 16 in 64 columns) and wide (rp > r) layouts"""
    from vt355 import ops
    g = torch.Generator().manual_seed(20 + r)
    sb = (torch.randn(N0, r, generator=g) * 0.1).to(BF)
    c = torch.rand(N0, generator=g) + 0.5
    e = torch.zeros(N0, ext, dtype=BF); e[:, :r] = sb
    # forward operand [N, K + ext]
    buf, body = _frame(dev, N0, K0 + ext, 8)
    base = (torch.randn(N0, K0, generator=g) * 0.02).to(BF)
    body[:, :K0] = base.to(dev); body[:, K0:] = e.to(dev)
    ops.dora_scale(body[:, K0:], body[:, K0:], c.to(dev))
    torch.cuda.synchronize()
    assert _same_bits(body[:, K0:].cpu(), _expect(e, c)) and _same_bits(body[:, :K0].cpu(), base)
    assert (body[:, K0 + r:] == 0).all() and (body[:, K0:K0 + r] != 0).any()
    untouched(buf, (slice(1, N0 + 1), slice(0, K0 + ext)), "in-place dora_scale wrote outside the operand")
    # transposed operand [K + ext, N]
    buf, body = _frame(dev, K0 + ext, N0, 8)
    body[:K0] = base.t().to(dev); body[K0:] = e.t().to(dev)
    ops.dora_scale(body[K0:], body[K0:], c.to(dev), by_col=True)
    torch.cuda.synchronize()
    assert _same_bits(body[K0:].cpu(), _expect(e.t(), c, by_col=True)) and _same_bits(body[:K0].cpu(), base.t())
    assert (body[K0 + r:] == 0).all()
    untouched(buf, (slice(1, K0 + ext + 1), slice(0, N0)), "in-place dora_scale wrote outside the operand")


@pytest.mark.parametrize("Nn,K", [(N0, K0), (64, 7680), (7680, 64)], ids=["200x192", "64x7680", "7680x64"])
def test_transpose_scale_is_one_rounding(dev, Nn, K):
    """dst[k, j] = bf16(c[j] * w[j, k]) bit for bit; [200, 192]: partial tiles on the source's row side; 7680: the feed-forward widths"""
    from vt355 import ops
    g = torch.Generator().manual_seed(31 + Nn)
    w = (torch.randn(Nn, K, generator=g) * 0.02).to(BF)
    c = torch.randn(Nn, generator=g)
    src = torch.full((Nn, K + 16), float("nan"), dtype=BF, device=dev); src[:, :K] = w.to(dev)
    buf, dst = _frame(dev, K, Nn, 24)
    ops.dora_transpose_scale(src[:, :K], dst, c.to(dev))
    torch.cuda.synchronize()
    assert _same_bits(dst.cpu(), _expect(w, c).t())
    untouched(buf, (slice(1, K + 1), slice(0, Nn)), "dora_transpose_scale wrote outside the operand")


def test_db_add_and_dm_finish(dev):
    from vt355 import ops
    g = torch.Generator().manual_seed(41)
    r = 20
    G, S, c = torch.randn(N0, r, generator=g), torch.randn(N0, r, generator=g), torch.rand(N0, generator=g) + 0.5
    Gd = G.to(dev)
    ops.dora_db_add(Gd, S.to(dev), c.to(dev))
    assert rel_l2(Gd, G.double() + c[:, None].double() * S.double()) < 2e-7          # two fp32 roundings per element
    sg, sgy, m = torch.randn(N0, generator=g), torch.randn(N0, generator=g), torch.rand(N0, generator=g) + 0.5
    b = torch.randn(N0, generator=g).to(BF)
    dm0 = torch.randn(N0, generator=g)
    dm = dm0.to(dev)
    ops.dora_dm(sg.to(dev), sgy.to(dev), b.to(dev), m.to(dev), dm)
    want = dm0.double() + (sgy.double() - b.double() * sg.double()) / m.double()
    assert rel_l2(dm, want) < 3e-7                # three fp32 roundings per element
    dm = dm0.to(dev)
    ops.dora_dm(sg.to(dev), sgy.to(dev), None, m.to(dev), dm)
    assert rel_l2(dm, dm0.double() + sgy.double() / m.double()) < 3e-7


def test_entry_points_refuse_bad_arguments(dev):
    from vt355 import ops
    from vt355._lib import VtError
    w = torch.zeros(64, 128 + 8, dtype=BF, device=dev); a = torch.zeros(136, 128, dtype=BF, device=dev)
    b = torch.zeros(64, 4, dtype=BF, device=dev); out = torch.zeros(64, device=dev); c = torch.ones(256, device=dev)
    ops.dora_norm(w[:, :128], a, b, 1, 4, 1.0, out)
    with pytest.raises(VtError):
        ops.dora_norm(w[:, 4:132], a, b, 1, 4, 1.0, out)                              # W not 16-byte aligned
    with pytest.raises(VtError):
        ops.dora_norm(w[:, :124], a[:, :124], b, 1, 4, 1.0, out)                      # K = 124 is no multiple of 8
    with pytest.raises(VtError):
        ops.dora_norm(w[:, :128], a, torch.zeros(64, 129, dtype=BF, device=dev), 1, 129, 1.0, out)      # r > 128
    with pytest.raises(VtError):
        ops.dora_norm(w[:60, :128], a, b[:60], 3, 4, 1.0, out)                        # 20 rows per adapter: no multiple of 8
    with pytest.raises(VtError):
        ops.dora_norm(w[:, :128], a, b, 4, 4, 1.0, out)                               # four adapters
    with pytest.raises(ValueError):
        ops.dora_norm(w[:, :128], a[:2], b, 1, 4, 1.0, out)                           # A has fewer than r rows
    with pytest.raises(ValueError):
        ops.dora_norm(w[:, :128], a, b, 1, 4, 1.0, out[:32])                          # out is shorter than the rows
    with pytest.raises(ValueError):
        ops.dora_norm(w[:, :128].cpu(), a, b, 1, 4, 1.0, out)                         # host tensor
    with pytest.raises(ValueError):
        ops.dora_norm(w[:, :128], a, b.float(), 1, 4, 1.0, out)                       # B is not bf16
    x = torch.zeros(64, 128 + 64, dtype=BF, device=dev)
    with pytest.raises(VtError):
        ops.dora_scale(x[:, 4:132], x[:, 4:132], c)                                   # not 16-byte aligned
    with pytest.raises(VtError):
        ops.dora_scale(x[:, 128:148], x[:, 128:148], c)                               # 20 extension columns: no multiple of 8
    with pytest.raises(VtError):
        ops.dora_scale(x[:, :128], x[:, :128], c[1:], by_col=True)                    # per-column factors not 16-byte aligned
    with pytest.raises(ValueError):
        ops.dora_scale(x[:, :128], x[:, :64], c)                                      # shapes differ
    with pytest.raises(ValueError):
        ops.dora_scale(x[:, :128], x[:, :128], c[:32])                                # fewer factors than rows
    with pytest.raises(ValueError):
        ops.dora_scale(x[:, :128], x[:, :128], c.cpu())                               # host tensor
    t = torch.zeros(128, 64 + 8, dtype=BF, device=dev)
    with pytest.raises(VtError):
        ops.dora_transpose_scale(x[:60, :128], t[:, :60], c)                          # 60 rows: no multiple of 8
    with pytest.raises(VtError):
        ops.dora_transpose_scale(x[:, :128], t[:, 4:68], c)                           # destination not 16-byte aligned
    with pytest.raises(ValueError):
        ops.dora_transpose_scale(x[:, :128], t[:64, :64], c)                          # destination is not [K, N]
    with pytest.raises(ValueError):
        ops.dora_transpose_scale(x[:, :128].cpu(), t[:, :64], c)                      # host tensor
    with pytest.raises(ValueError):
        ops.dora_db_add(torch.zeros(64, 4, device=dev), torch.zeros(64, 8, device=dev), c)
    with pytest.raises(VtError):
        ops.dora_db_add(torch.zeros(64, 129, device=dev), torch.zeros(64, 129, device=dev), c)          # r > 128
    with pytest.raises(ValueError):
        ops.dora_dm(out, out, None, out[:32], torch.zeros(64, device=dev))            # a vector shorter than dm


# ================================================================== the model
def _device_step(dev, r, targets=SIX, rope=False, recompute="never", **build_kw):
    """selfcheck.tiny_train_step_check's step (B = 2, 2 layers) with DoRA adapters at dora_ref's step inputs"""
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    cfg, model, peft, st = R.build_tiny(dev, targets, lora_r=r, use_rotary_positional_embeddings=rope, **build_kw)
    model.enable_gradient_checkpointing(recompute)
    x0, text, noise, t = R.tiny_inputs(cfg)
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
    tabs = R.rope_tables(cfg, rope)
    sa, sb, w = sched.coefficients(t.to(dev))

    def run(zero=True):
        if zero:
            st.grad.zero_()
        out = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev), return_dict=False,
                   image_rotary_emb=None if tabs is None else (tabs[0].to(dev), tabs[1].to(dev)))[0]
        loss = _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w)
        loss.backward()
        return loss.item(), R.device_grads(st), out
    return dict(cfg=cfg, model=model, peft=peft, st=st, run=run, x0=x0, text=text, t=t, tabs=tabs, noisy=noisy.float().cpu().double())


def _ref(monkeypatch, s, variant="right", params=None):
    return R.reference_step(monkeypatch, s["cfg"], s["model"], s["st"], s["noisy"], s["x0"], s["text"], s["t"], variant, s["tabs"], params)


STEP_CASES = [(4, ATTN, False), (4, SIX, False), (16, SIX, False), (20, SIX, False), (40, SIX, False), (128, SIX, False), (4, SIX, True),
              (4, ["ff.net.2"], False)]
GROUP = {"norm_attached": R.adapter_names, "bias_scaled": R.mag_names, "norm_of_w": R.adapter_names}


@pytest.mark.parametrize("r,targets,rope", STEP_CASES, ids=[f"r{r}_{len(tg)}targets{'_rope' if rp else ''}" for r, tg, rp in STEP_CASES])
def test_train_step_matches_the_reference(dev, r, targets, rope, monkeypatch):
    """loss and every gradient (A, B and the magnitudes) of the tiny training step against the fp64 restatement at tiny_train_step_check's
    bars: loss 2e-2 relative, gradients rel-L2 6e-2 and cosine > 0.995, over all parameters and over the magnitudes alone; every gradient
    is non-zero.  r = 4, 16: narrow; 20, 40, 128: wide.  Each wrong restatement must fail the same bars on the group it touches
    (tests/test_dora_cpu.py shows that the inputs separate them)."""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, targets, rope)
    loss, grads, _ = s["run"]()
    loss_ref, gref, _ = _ref(monkeypatch, s)
    assert set(grads) == set(gref)
    mag = R.mag_names(gref)
    assert len(mag) == 2 * len(targets) and all(gref[k].abs().max().item() > 0 and grads[k].abs().max().item() > 0 for k in gref)
    rel, cos = R.overall(R.flat(grads, list(gref)), R.flat(gref))
    relm, cosm = R.overall(R.flat(grads, mag), R.flat(gref, mag))
    worst = max((rel_l2(grads[k], gref[k]), k) for k in gref)
    print(f"r={r} targets={len(targets)} rope={rope}: loss {loss:.6f} ref {loss_ref:.6f}; grads rel-L2 {rel:.3e} cos {cos:.5f}; "
          f"magnitudes rel-L2 {relm:.3e} cos {cosm:.5f}; worst parameter {worst[0]:.3e} {worst[1]}")
    assert abs(loss - loss_ref) / abs(loss_ref) < 2e-2, (loss, loss_ref)
    assert rel < 6e-2 and cos > 0.995, (rel, cos)
    assert relm < 6e-2 and cosm > 0.995, (relm, cosm)
    for variant in R.VARIANTS[1:]:
        _, gw, _ = _ref(monkeypatch, s, variant)
        names = GROUP[variant](gref)
        relw, cosw = R.overall(R.flat(grads, names), R.flat(gw, names))
        print(f"   against {variant}: rel-L2 {relw:.3e} cos {cosw:.5f}")
        assert not (relw < 6e-2 and cosw > 0.995), (variant, relw, cosw)


@pytest.mark.parametrize("r", [4, 40])
def test_gradients_accumulate_across_micro_batches(dev, r, monkeypatch):
    """a second backward without zeroing doubles every gradient (+= semantics of dA, dB through the scratch, and dm)"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r)
    _, g1, _ = s["run"]()
    _, g2, _ = s["run"](zero=False)
    assert rel_l2(R.flat(g2), 2 * R.flat(g1)) < 1e-3          # fp32 atomics differ in order between the two passes


@pytest.mark.parametrize("r", [4, 40])
def test_peft_init_is_the_base_model(dev, r, monkeypatch):
    """B = 0 and untouched magnitudes (m from the norm kernel): c == 1.0f, the prediction is torch.equal to the one of the same base
    weights without any adapter; dA is exactly 0, dB and dm are not"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    from selfcheck import CFG_KEYS
    from vt355.dit import CogVideoXTransformer3DModel
    s = _device_step(dev, r, b_std=0.0, m_std=0.0, bias_gain=1.0)
    _, g, out = s["run"]()
    for L in s["model"]._packed.layers:
        for c in (L.c_qkv, L.c_o, L.c_1, L.c_2):
            assert (c == 1.0).all()
    base = CogVideoXTransformer3DModel(**{k: getattr(s["cfg"], k) for k in CFG_KEYS}).init_weights(0).to(dev)
    base.requires_grad_(False)
    with torch.no_grad():
        out_base = base(hidden_states=s["noisy"].to(dev, BF), encoder_hidden_states=s["text"].to(dev), timestep=s["t"].to(dev),
                        return_dict=False)[0]
    assert torch.equal(out, out_base)
    for k in g:
        if "lora_A" in k:
            assert (g[k] == 0).all(), k
        else:
            assert g[k].abs().max().item() > 0, k


@pytest.mark.parametrize("r", [4, 40])
def test_recompute_gives_the_same_loss_and_gradients(dev, r, monkeypatch):
    """enable_gradient_checkpointing("always") rebuilds ao / fo with the rest of the block: the same loss bits, gradients within rel-L2
    1e-3 (the siblings' tolerance), over all parameters and over the magnitudes"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r)
    l0, g0, _ = s["run"]()
    s["model"].enable_gradient_checkpointing("always")
    l1, g1, _ = s["run"]()
    assert l0 == l1
    mag = R.mag_names(g0)
    assert R.flat(g0, mag).abs().max().item() > 0
    assert rel_l2(R.flat(g1), R.flat(g0)) < 1e-3 and rel_l2(R.flat(g1, mag), R.flat(g0, mag)) < 1e-3


@pytest.mark.parametrize("r", [4, 40])
def test_two_steps_with_fused_adamw_refresh_the_operands(dev, r, monkeypatch):
    """FusedAdamW over the one flat buffer moves the magnitudes with the adapters; the forward after the step runs on refreshed operands:
    its loss matches the restatement at the read-back parameters (2e-2, the step's bar) and its prediction is closer to that restatement
    than to the one at the parameters before the step (stale operands would give the reverse); a further forward without a step does not
    repack"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    from vt355 import ops
    from vt355.optim import FusedAdamW
    s = _device_step(dev, r)
    st, model = s["st"], s["model"]
    opt = FusedAdamW(st.params, lr=2e-2, weight_decay=0.0, lora_state=st)
    old = R.oracle_params(model, st)
    _, _, out_old_ref = _ref(monkeypatch, s, params=old)
    m0 = torch.cat([st.view(st.flat, i, "M", 3) for i in range(st.L)]).clone()
    s["run"]()
    v0 = model._packed.lora_version
    opt.step()
    assert not torch.equal(torch.cat([st.view(st.flat, i, "M", 3) for i in range(st.L)]), m0)
    loss1, _, out1 = s["run"]()
    assert model._packed.lora_version == st.version != v0
    loss_ref, _, out_new_ref = _ref(monkeypatch, s)
    rel_new, rel_old = rel_l2(out1, out_new_ref), rel_l2(out1, out_old_ref)
    print(f"r={r}: loss {loss1:.6f} ref {loss_ref:.6f}; prediction against the restatement after / before the step: {rel_new:.3e} / {rel_old:.3e}")
    assert abs(loss1 - loss_ref) / abs(loss_ref) < 2e-2
    assert rel_new < 0.5 * rel_old
    calls = []
    monkeypatch.setattr(ops, "dora_norm", lambda *a, **k: calls.append(1))
    v1 = model._packed.lora_version
    _, _, out2 = s["run"]()
    assert model._packed.lora_version == v1 == st.version and not calls
    assert torch.equal(out2, out1)


def test_checkpoint_round_trip_reproduces_the_prediction(dev, tmp_path, monkeypatch):
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    from types import SimpleNamespace
    from vt355 import checkpoint as C
    from vt355.workflow import CogVideoXWorkFlow
    src = _device_step(dev, 4)
    _, _, out_src = src["run"]()
    wf = SimpleNamespace(model=src["peft"], global_step=1)
    wf.on_save_checkpoint = lambda ck: CogVideoXWorkFlow.on_save_checkpoint(wf, ck)
    path = C.save_checkpoint(wf, str(tmp_path / "last.ckpt"), epoch=0)
    sd = C.load_checkpoint_file(path)["state_dict"]
    assert all("lora" in k for k in sd) and sum("lora_magnitude_vector" in k for k in sd) == 12
    dst = _device_step(dev, 4, b_std=0.0, m_std=0.0)
    _, _, out_init = dst["run"]()
    assert not torch.equal(out_init, out_src)
    assert C.load_lora_from_ckpt(dst["peft"], path) == 36
    _, _, out_dst = dst["run"]()
    assert torch.equal(out_dst, out_src)


def test_model_injected_on_the_cpu_and_moved_keeps_its_magnitudes(dev, monkeypatch):
    """get_peft_model on a CPU model (m = torch's fp32 row norm), then .to(device): on_module_moved re-homes the magnitudes with the
    adapters into one flat buffer; c is 1 to the fp32 rounding of two different summation orders, not bit-exactly: torch's norm 1.46e-7, the
    kernel's bar 2.92e-7 (test_norm_randn_against_fp64) and the division's 6e-8 add to 5e-7"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    from vt355 import engine
    cfg, model, peft, st = R.build_tiny(torch.device("cpu"), b_std=0.0, m_std=0.0)
    m_cpu = torch.cat([st.view(st.flat, i, "M", j) for i in range(st.L) for j in range(6)]).clone()
    peft.to(dev)
    st = model.lora
    assert st.flat.is_cuda and st.flat.numel() == st.numel and st.grad.is_cuda
    for p, (layer, kind, j) in zip(st.params, st._index):
        assert p.data_ptr() == st.view(st.flat, layer, kind, j).data_ptr() and p.grad.data_ptr() == st.view(st.grad, layer, kind, j).data_ptr()
    assert torch.equal(torch.cat([st.view(st.flat, i, "M", j) for i in range(st.L) for j in range(6)]).cpu(), m_cpu)
    P = engine.packed(model)
    for L in P.layers:
        for c in (L.c_qkv, L.c_o, L.c_1, L.c_2):
            assert (c - 1).abs().max().item() < 5e-7
