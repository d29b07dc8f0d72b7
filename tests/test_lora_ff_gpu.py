"""LoRA on the CogVideoX feed-forward pair ff.net.0.proj / ff.net.2 on the GPU: the two dgelu forms of the dropped dX correction
(csrc/lora.hip, csrc/lora_wide.hip) through vt355.ops, and the training step through the module interface against the fp64 restatement
of tests/lora_ff_ref.py.

Exact kernel tests follow tests/test_lora_dropout_gpu.py: small-integer dT, A, dX, with U = 0 (gelu'(0) = 0.5) and p = 0.5 (1 / (1 - p)
= 2), so the factor is exactly 1 and dX + keep * (dT A) is an integer that fp32 and bf16 hold exactly (|result| <= 256 asserted on the
reference); compared bit for bit.  The expected masks are oracle/philox.py's on the LOGICAL width K (e = m * K + k), whatever ldx / ldu."""
import pytest
import torch

import lora_ff_ref as R
from parity import close, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
NAN = float("nan")
SENT = 768.0
SEED, SITE0 = R.SEED, 116 + 7          # a feed-forward site of a deep layer: the upper word of the Philox counter is non-zero
M0, K0 = 200, 192                      # M: a 128-row block and 72 rows (wide), three 64-row groups and 8 rows; K: three 64-column steps
SIX = list(R.TARGETS)


def rb(x):
    return x.to(BF).float()


def ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def sparse_ints(g, lo, hi, keep_one_in, *shape):
    return ints(g, lo, hi, *shape) * (torch.randint(0, keep_one_in, shape, generator=g) == 0).double()


def mask(M, K, p, site):
    return R.keep_mask(M, K, p, SEED, site)


def dgelu64(u):
    """tanh-GELU's derivative in fp64, by autograd on the oracle's gelu_tanh"""
    import cogvideox_oracle as O
    x = u.clone().double().requires_grad_(True)
    O.gelu_tanh(x).sum().backward()
    return x.grad


def layout(n, r):
    rp = (r + 15) // 16 * 16
    return rp, (n * rp + 63) // 64 * 64


def ref_up(dx, dt, A, u, n, r, rp, p, K, site0=SITE0):
    """dX + gelu'(U) / (1 - p) * sum_j keep_j * (dT_j A_j); adapter j = columns [j rp, j rp + r) of dT"""
    out = dx.clone()
    g = dgelu64(u)
    for j in range(n):
        out += g * mask(dx.shape[0], K, p, site0 + j) * (dt[:, j * rp:j * rp + r] @ A[j * r:(j + 1) * r]) / (1 - p)
    return out


def launch(dev, dx, dt, A, u, n, r, rp, p, K, wide, ldx_pad=64, ldu_pad=24, site0=SITE0):
    """runs the kernel on sentinel-framed buffers (dX | dT in one buffer with ldx > K, U with a row stride of its own, NaN padding);
    returns the new dX columns and checks what must not change"""
    from vt355 import ops
    M = dx.shape[0]
    ext = dt.shape[1]
    buf = torch.full((M + 2, K + max(ext, ldx_pad)), NAN, dtype=BF, device=dev)
    buf[0] = SENT; buf[-1] = SENT
    body = buf[1:M + 1]
    body[:, :K] = dx.to(dev, BF); body[:, K:K + ext] = dt.to(dev, BF)
    ub = torch.full((M, K + ldu_pad), NAN, dtype=BF, device=dev)
    ub[:, :K] = u.to(dev, BF)
    ext_before = body[:, K:].contiguous().view(torch.int16).cpu()
    u_before = ub.contiguous().view(torch.int16).cpu()
    Ad = A.to(dev, BF)
    if wide:
        ops.lora_up_add_wide_dgelu_drop(body, body[:, K:], Ad, n, r, rp, ub[:, :K], K, p, SEED, site0)
    else:
        ops.lora_up_add_dgelu_drop(body, body[:, K:], Ad, n * r, n, ub[:, :K], K, p, SEED, site0)
    torch.cuda.synchronize()
    assert torch.equal(body[:, K:].contiguous().view(torch.int16).cpu(), ext_before), "the extension columns changed"
    assert torch.equal(ub.contiguous().view(torch.int16).cpu(), u_before), "U changed"
    assert (buf[0] == SENT).all() and (buf[-1] == SENT).all(), "wrote outside the M rows"
    return body[:, :K]


# ================================================================== exact
@pytest.mark.parametrize("Rr,n", [(4, 1), (16, 1), (12, 3)], ids=["R4", "R16", "R4x3"])
def test_up_add_dgelu_drop_exact_narrow(dev, Rr, n):
    """M = 200, K = 192, ldx = 256, ldu = 216.  dX in [-3, 3], dT in {-1, 0, 1}, A in [-2, 2]: |dT A| <= 32.  R = 4 x 3: three adapters
    under three masks in one call (the feed-forward Linears have one; the template keeps the siblings' adapter loop)."""
    g = torch.Generator().manual_seed(300 + Rr)
    dx, dt, A = ints(g, -3, 3, M0, K0), ints(g, -1, 1, M0, Rr), ints(g, -2, 2, Rr, K0)
    u = torch.zeros(M0, K0)
    got = launch(dev, dx, dt, A, u, n, Rr // n, Rr // n, 0.5, K0, wide=False).float().cpu().double()
    ref = dx.clone()
    for j in range(n):
        r = Rr // n
        ref += mask(M0, K0, 0.5, SITE0 + j) * (dt[:, j * r:(j + 1) * r] @ A[j * r:(j + 1) * r])
    assert ref.abs().max().item() <= 256
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} differ"
    assert not torch.equal(ref, dx + dt @ A) and not torch.equal(ref, dx)


@pytest.mark.parametrize("r,rp,n", [(20, 32, 1), (40, 48, 1), (128, 128, 1), (40, 48, 3)], ids=["r20", "r40", "r128", "r40x3"])
def test_up_add_dgelu_drop_exact_wide(dev, r, rp, n):
    """M = 200 (a 128-row block and 72 rows: wave 2 of the second block has 8 rows, wave 3 none), K = 192; dT and A in {-1, 0, 1} with
    one in two / four entries non-zero keep |result| <= 256 (asserted)"""
    _, ext = layout(n, r)
    g = torch.Generator().manual_seed(400 + r + n)
    dx, A = ints(g, -3, 3, M0, K0), sparse_ints(g, -1, 1, 4, n * r, K0)
    dt = torch.zeros(M0, ext, dtype=torch.float64)
    for j in range(n):
        dt[:, j * rp:j * rp + r] = sparse_ints(g, -1, 1, 2, M0, r)
    u = torch.zeros(M0, K0)
    got = launch(dev, dx, dt, A, u, n, r, rp, 0.5, K0, wide=True).float().cpu().double()
    ref = dx.clone()
    for j in range(n):
        ref += mask(M0, K0, 0.5, SITE0 + j) * (dt[:, j * rp:j * rp + r] @ A[j * r:(j + 1) * r])
    assert ref.abs().max().item() <= 256
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} differ"
    assert not torch.equal(ref, dx + dt[:, :r] @ A[:r]) and not torch.equal(ref, dx)


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_up_add_dgelu_drop_counter_arithmetic_at_k7680(dev, wide):
    """K = 7680 = 4 x 1920 (the 2B model's feed-forward width), M = 64: the element index e = m * K + k of the mask at the width the
    engine runs ff.net.2's correction at"""
    M, K = 64, 7680
    r, rp = (20, 32) if wide else (4, 4)
    g = torch.Generator().manual_seed(7680 + wide)
    dx, A, dt = ints(g, -3, 3, M, K), sparse_ints(g, -1, 1, 2, r, K), torch.zeros(M, 64, dtype=torch.float64)
    dt[:, :r] = ints(g, -1, 1, M, r)
    got = launch(dev, dx, dt, A, torch.zeros(M, K), 1, r, rp, 0.5, K, wide=wide).float().cpu().double()
    ref = dx + mask(M, K, 0.5, SITE0) * (dt[:, :r] @ A)
    assert ref.abs().max().item() <= 256
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} of {ref.numel()} differ"


# ================================================================== randn against fp64
@pytest.mark.parametrize("wide,r,rp", [(False, 4, 4), (False, 16, 16), (True, 20, 32), (True, 40, 48), (True, 128, 128)])
@pytest.mark.parametrize("zero_dx", [False, True], ids=["randn_dx", "zero_dx_u_spread"])
def test_up_add_dgelu_drop_randn(dev, wide, r, rp, zero_dx):
    """p = 0.1 against fp64 on the bf16-rounded operands at the siblings' bars (test_lora_up_add_drop_randn / test_wide_drop_randn: rtol
    1e-2, atol 2e-2).  zero_dx: dX = 0 and U spread over [-3, 3], where gelu' runs from -0.13 to 1.13: a missing or misplaced gelu' is an
    O(1) error of the whole result."""
    g = torch.Generator().manual_seed(500 + r)
    _, ext = layout(1, r)
    A = rb(torch.randn(r, K0, generator=g) * 0.1).double()
    dt = torch.zeros(M0, ext if wide else 16, dtype=torch.float64)
    dt[:, :r] = rb(torch.randn(M0, r, generator=g)).double()
    if zero_dx:
        dx = torch.zeros(M0, K0, dtype=torch.float64)
        u = rb(torch.linspace(-3, 3, M0 * K0)[torch.randperm(M0 * K0, generator=g)].view(M0, K0)).double()
    else:
        dx = rb(torch.randn(M0, K0, generator=g)).double()
        u = rb(torch.randn(M0, K0, generator=g)).double()
    got = launch(dev, dx, dt, A, u, 1, r, rp, 0.1, K0, wide=wide)
    ref = ref_up(dx, dt, A, u, 1, r, rp, 0.1, K0)
    close(got, ref, 1e-2, 2e-2, f"up_add_dgelu_drop wide={wide} r={r}")
    if zero_dx:
        plain = mask(M0, K0, 0.1, SITE0) * (dt[:, :r] @ A) / 0.9          # the sibling's result: no gelu'
        assert rel_l2(plain, ref) > 0.3, "the inputs do not tell a missing gelu' from the right result"
        assert rel_l2(got.float().cpu().double(), ref) < 1e-2


# ================================================================== the mask, from a second source on the device
@pytest.mark.parametrize("p", [0.5, 0.1])
def test_kernel_masks_equal_vt_dropout_bf16(dev, p):
    """dX = 0, U = 0, dT = e_0 and A[0] = 1 make the result keep(m, k) * 0.5 / (1 - p): the mask the kernels imply must be the one
    vt_dropout_bf16 exports at the same (seed, offset = site << 36)"""
    from vt355 import ops
    from parity import poisoned
    ones = torch.ones(M0, K0, dtype=BF, device=dev)
    y = poisoned((M0, K0), BF, dev); mk = poisoned((M0, K0), torch.uint8, dev)
    ops.dropout(ones, y, p, SEED, offset=SITE0 << 36, mask_out=mk)
    for wide, r, rp in ((False, 4, 4), (True, 20, 32)):
        dt = torch.zeros(M0, 64, dtype=torch.float64); dt[:, 0] = 1
        A = torch.zeros(r, K0, dtype=torch.float64); A[0] = 1
        got = launch(dev, torch.zeros(M0, K0, dtype=torch.float64), dt, A, torch.zeros(M0, K0), 1, r, rp, p, K0, wide=wide)
        implied = (got != 0).to(torch.uint8)
        assert torch.equal(implied, mk), f"wide={wide}: {(implied != mk).sum().item()} mask bits differ from vt_dropout_bf16's"
        assert torch.equal(got.float().cpu(), (0.5 * y.float()).cpu()), "kept elements are not 0.5 / (1 - p) rounded once"
    assert 0 < mk.sum().item() < mk.numel()


def test_entry_points_refuse_bad_arguments(dev):
    from vt355 import ops
    from vt355._lib import VtError
    x = torch.zeros(64, 128 + 64, dtype=BF, device=dev); a = torch.zeros(32, 128, dtype=BF, device=dev)
    u = torch.zeros(64, 136, dtype=BF, device=dev)
    for p in (1.0, -0.1, float("nan")):
        with pytest.raises(VtError):
            ops.lora_up_add_dgelu_drop(x, x[:, 128:], a, 4, 1, u, 128, p, 1, 0)
        with pytest.raises(VtError):
            ops.lora_up_add_wide_dgelu_drop(x, x[:, 128:], a, 1, 20, 32, u, 128, p, 1, 0)
    with pytest.raises(VtError):
        ops.lora_up_add_dgelu_drop(x, x[:, 128:], a, 12, 5, u, 128, 0.1, 1, 0)            # 12 rank rows do not split into 5 adapters
    with pytest.raises(VtError):
        ops.lora_up_add_dgelu_drop(x, x[:, 128:], a, 17, 1, u, 128, 0.1, 1, 0)            # the narrow kernel takes 16 rank rows
    with pytest.raises(VtError):
        ops.lora_up_add_dgelu_drop(x, x[:, 128:], a, 4, 1, u[:, 4:], 128, 0.1, 1, 0)      # U not 16-byte aligned
    with pytest.raises(VtError):
        ops.lora_up_add_wide_dgelu_drop(x, x[:, 128:], a, 1, 20, 24, u, 128, 0.1, 1, 0)   # rp is no multiple of 16
    with pytest.raises(VtError):
        ops.lora_up_add_wide_dgelu_drop(x, x[:, 128:], a, 1, 20, 32, u[:, 2:], 128, 0.1, 1, 0)   # U not 8-byte aligned
    with pytest.raises(VtError):
        ops.lora_up_add_wide_dgelu_drop(x, x[:, 128:], a, 1, 20, 32, u, 128, 0.1, 1, -1)  # negative site
    with pytest.raises(ValueError):
        ops.lora_up_add_dgelu_drop(x, x[:, 128:], a, 4, 1, u[:32], 128, 0.1, 1, 0)        # U has fewer rows than dX
    with pytest.raises(ValueError):
        ops.lora_up_add_wide_dgelu_drop(x, x[:, 128:], a, 1, 20, 32, u[:, :64], 128, 0.1, 1, 0)   # U has fewer than K columns
    with pytest.raises(ValueError):
        ops.lora_up_add_wide_dgelu_drop(x, x[:, 128:], a[:16], 1, 20, 32, u, 128, 0.1, 1, 0)      # A has fewer than r rows
    with pytest.raises(ValueError):
        ops.lora_up_add_dgelu_drop(x, x[:, 128:], a, 4, 1, u.float(), 128, 0.1, 1, 0)     # U is not bf16
    with pytest.raises(ValueError):
        ops.lora_up_add_dgelu_drop(x.cpu(), x[:, 128:], a, 4, 1, u, 128, 0.1, 1, 0)       # host tensor


# ================================================================== the model
def _device_step(dev, r, p, rope=False, targets=SIX, b_random=True, recompute="never", scaling=0.25):
    """selfcheck.tiny_train_step_check's step (B = 2, 2 layers) with the given targets, lora_dropout p and a pinned seed"""
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    cfg, model, peft, st = R.build_tiny(dev, targets, lora_r=r, lora_b_random=b_random, p=p, scaling=scaling,
                                        use_rotary_positional_embeddings=rope)
    model.lora_dropout_seed = SEED
    model.enable_gradient_checkpointing(recompute)
    x0, text, noise, t = R.tiny_inputs(cfg)
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0.to(dev), noise.to(dev), t.to(dev))
    tabs = R.rope_tables(cfg, rope)
    sa, sb, w = sched.coefficients(t.to(dev))

    def run():
        st.grad.zero_()
        out = peft(hidden_states=noisy, encoder_hidden_states=text.to(dev), timestep=t.to(dev), return_dict=False,
                   image_rotary_emb=None if tabs is None else (tabs[0].to(dev), tabs[1].to(dev)))[0]
        loss = _LossFn.apply(out, noisy, x0.to(dev), sa, sb, w)
        loss.backward()
        return loss.item(), R.device_grads(st), out
    return dict(cfg=cfg, model=model, peft=peft, st=st, run=run, x0=x0, text=text, t=t, tabs=tabs, noisy=noisy.float().cpu().double())


STEP_CASES = [(4, 0.0, False, SIX), (16, 0.0, False, SIX), (20, 0.0, False, SIX), (40, 0.0, False, SIX), (128, 0.0, False, SIX),
              (4, 0.1, False, SIX), (4, 0.5, False, SIX), (40, 0.1, False, SIX), (40, 0.5, False, SIX),
              (4, 0.1, True, SIX), (4, 0.1, False, ["ff.net.2"]), (4, 0.0, False, ["ff.net.2"])]


@pytest.mark.parametrize("r,p,rope,targets", STEP_CASES,
                         ids=[f"r{r}_p{p}{'_rope' if rope else ''}{'_ff2only' if len(tg) == 1 else ''}" for r, p, rope, tg in STEP_CASES])
def test_train_step_matches_the_reference(dev, r, p, rope, targets, monkeypatch):
    """loss and every adapter gradient of the tiny training step (B = 2, 2 layers, random B, pinned seed) against the fp64 restatement, at
    tiny_train_step_check's bars: loss 2e-2 relative, gradients rel-L2 6e-2 and cosine > 0.995, over all adapters and over the
    feed-forward adapters alone.  r = 4, 16: narrow; 20 (rp = 32), 40 (rp = 48), 128: wide; p = 0: ff.net.2's dX correction rides in the
    K-extension of the dGELU product; p > 0: the dgelu_drop kernels.  At p = 0.5 (lora_alpha = 4 r, see lora_ff_ref.WRONG_SCALING) each
    wrong reference must fail the same bars on the feed-forward group."""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, p, rope, targets, scaling=R.WRONG_SCALING if p == 0.5 else 0.25)
    loss, grads, _ = s["run"]()
    if p > 0:
        assert s["model"].last_lora_dropout_seed == SEED
    ref = lambda variant: R.reference_step(monkeypatch, s["cfg"], s["model"], s["st"], s["noisy"], s["x0"], s["text"], s["t"], p, SEED,
                                           variant, s["tabs"])
    loss_ref, gref, _ = ref("right")
    assert set(grads) == set(gref)
    ff = R.ff_names(gref)
    assert len(ff) == (8 if len(targets) == 6 else 4) and all(gref[k].abs().max().item() > 0 for k in gref)
    rel, cos = R.overall(R.flat(grads, list(gref)), R.flat(gref))
    relf, cosf = R.overall(R.flat(grads, ff), R.flat(gref, ff))
    worst = max((rel_l2(grads[k], gref[k]), k) for k in gref)
    print(f"r={r} p={p} rope={rope} targets={len(targets)}: loss {loss:.6f} ref {loss_ref:.6f}; grads rel-L2 {rel:.3e} cos {cos:.5f}; "
          f"feed-forward group rel-L2 {relf:.3e} cos {cosf:.5f}; worst adapter {worst[0]:.3e} {worst[1]}")
    assert abs(loss - loss_ref) / abs(loss_ref) < 2e-2, (loss, loss_ref)
    assert rel < 6e-2 and cos > 0.995, (rel, cos)
    assert relf < 6e-2 and cosf > 0.995, (relf, cosf)
    if p == 0.5:
        for variant in R.VARIANTS[1:]:
            _, gw, _ = ref(variant)
            relw, cosw = R.overall(R.flat(grads, ff), R.flat(gw, ff))
            print(f"   against {variant}: feed-forward group rel-L2 {relw:.3e} cos {cosw:.5f}")
            assert not (relw < 6e-2 and cosw > 0.995), (variant, relw, cosw)


@pytest.mark.parametrize("r,p", [(4, 0.0), (4, 0.1), (40, 0.1)])
def test_recompute_gives_the_same_loss_and_gradients(dev, r, p, monkeypatch):
    """enable_gradient_checkpointing("always") rebuilds x2 / gact (and their K-extensions) in the backward pass with the forward's dropout
    seed: the same loss bits, gradients within rel-L2 1e-3 (test_block_recompute_gives_the_same_gradients' tolerance)"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, p)
    l0, g0, _ = s["run"]()
    s["model"].enable_gradient_checkpointing("always")
    l1, g1, _ = s["run"]()
    assert l0 == l1
    ff = R.ff_names(g0)
    assert R.flat(g0, ff).abs().max().item() > 0
    assert rel_l2(R.flat(g1), R.flat(g0)) < 1e-3 and rel_l2(R.flat(g1, ff), R.flat(g0, ff)) < 1e-3


@pytest.mark.parametrize("r", [4, 40])
def test_eval_equals_p0_bit_for_bit(dev, r, monkeypatch):
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    s = _device_step(dev, r, 0.1)
    peft, model, st = s["peft"], s["model"], s["st"]
    _, _, out_train = s["run"]()
    st.p = 0.0
    _, g_nodrop, out_nodrop = s["run"]()
    assert not torch.equal(out_train, out_nodrop)
    st.p = 0.1
    peft.eval()
    assert not model.training
    _, g_eval, out_eval = s["run"]()
    assert torch.equal(out_eval, out_nodrop)
    with torch.no_grad():
        out_ng = peft(hidden_states=s["noisy"].to(dev, BF), encoder_hidden_states=s["text"].to(dev), timestep=s["t"].to(dev),
                      return_dict=False)[0]
    assert torch.equal(out_ng, out_nodrop)
    assert rel_l2(R.flat(g_eval), R.flat(g_nodrop)) < 1e-3          # the same kernels; fp32 atomics differ in order


@pytest.mark.parametrize("r", [4, 40])
def test_zero_b_leaves_the_base_models_prediction(dev, r, monkeypatch):
    """peft's init (B = 0): the prediction is torch.equal to the one of the same base weights without any adapter, in training mode with
    lora_dropout too; dA is exactly 0 and dB is not"""
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False); monkeypatch.delenv("VT355_RECOMPUTE", raising=False)
    from selfcheck import CFG_KEYS
    from vt355.dit import CogVideoXTransformer3DModel
    s = _device_step(dev, r, 0.1, b_random=False)
    _, g, out = s["run"]()
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
