"""HunyuanVideo lora_dropout on the device: the origin-map (_at) kernels against the unsharded identity-map calls bit for bit, train steps
against the fp64 shim reference of tests/hunyuan_lora_dropout_ref.py (all eight targets, ranks 4 / 24 / 128) and against its wrong
variants, the default path, seeds, the fp8 modes, the whole model and Ulysses sequence parallelism.  The tiny trunk of
tests/test_hunyuan_lora_ff_gpu.py: D 256, 2 heads, 4D 1024; 1 double + 1 single block; B 2, 160 image + 32 text rows, valid text lengths
32 / 19; every engine buffer starts out poisoned."""
import functools
import os

import numpy as np
import pytest
import torch

from hunyuan_lora_dropout_ref import keep_mask, reference_step, verdict
from hunyuan_lora_ff_ref import ALL, FF
from parity import poisoned, rel_l2
from test_hunyuan_lora_ff_gpu import _blocks, _inputs, _oracle_weights, _poison_engine

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D, H, M4 = 256, 2, 1024
B, LI, LT, VALID = 2, 160, 32, (32, 19)
P_DROP, SEED = 0.3, 1234


@pytest.fixture(autouse=True)
def _poisoned_buffers(monkeypatch):
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    _poison_engine(monkeypatch.setattr)


# ---------------------------------------------------------------------------------------------------------------- 1: the origin map
# Two ranks of a sequence-parallel single block: per sample 80 of the 160 image rows, then the 32 text rows.  A rank's 224 local rows
# are two segments of 112: the segment boundary (row 112) falls inside the second 64-row block, the last block (rows 192..223) is partial.
SEGL, SEGG, NFIRST, WORLD = 80 + 32, 160 + 32, 80, 2
MG, ML = 2 * SEGG, 2 * SEGL


def _rows_of(rank):
    """the unsharded rows that rank `rank` holds, in its local order"""
    return torch.tensor([b * SEGG + (rank * NFIRST + l if l < NFIRST else l + 160 - NFIRST) for b in range(2) for l in range(SEGL)])


def _origin(rank, k0, klog):
    return (SEGL, SEGG, NFIRST, rank * NFIRST, 160 - NFIRST, k0, klog)


COLS = [(256, 0, 256), (1024, 256, 1280)]          # (K of the call, k0, K_log): a whole input; the MLP columns of linear2's [M, 5 D] input


@pytest.mark.parametrize("K,k0,klog", COLS, ids=["K256", "K1024at256of1280"])
@pytest.mark.parametrize("n,r", [(1, 4), (3, 4), (1, 24), (3, 24)], ids=["n1r4", "n3r4", "n1r24", "n3r24"])
def test_at_kernels_equal_the_unsharded_identity_calls(dev, n, r, K, k0, klog):
    """down, up_add and its dgelu form on a rank's rows (and, in the second column case, on a column range) give the bits the identity-map
    call on the whole logical operand gives on those rows / columns"""
    from vt355 import ops
    rp, site0 = (r + 15) // 16 * 16, 5
    ext = (n * rp + 63) // 64 * 64
    gen = torch.Generator().manual_seed(100 * n + r + K)
    X = torch.randn(MG, klog, generator=gen).to(BF).to(dev)
    A = torch.zeros(n * r, klog, dtype=BF, device=dev)
    A[:, k0:k0 + K] = (torch.randn(n * r, K, generator=gen) * K ** -0.5).to(BF).to(dev)        # zero outside the call's columns: exact zeros in the sums
    # --- down: T over the logical input with A zero outside [k0, k0 + K) == T over the column range
    Tg = poisoned((MG, ext), BF, dev)
    ops.lora_down_wide_drop(X, A, n, r, rp, ext, Tg, klog, P_DROP, SEED, site0)
    assert torch.isfinite(Tg.float()).all() and Tg.float().abs().max().item() > 0
    dT = (torch.randn(MG, ext, generator=gen) * 0.1).to(BF).to(dev)
    dXg0 = torch.randn(MG, klog, generator=gen).to(BF).to(dev)
    U = torch.randn(MG, klog, generator=gen).to(BF).to(dev)
    Afull = (torch.randn(n * r, klog, generator=gen) * 0.1).to(BF).to(dev)
    dXg, dXgg = dXg0.clone(), dXg0.clone()
    ops.lora_up_add_wide_drop(dXg, dT, Afull, n, r, rp, klog, P_DROP, SEED, site0)
    ops.lora_up_add_wide_dgelu_drop(dXgg, dT, Afull, n, r, rp, U, klog, P_DROP, SEED, site0)
    assert not torch.equal(dXg, dXg0) and not torch.equal(dXgg, dXg) and torch.isfinite(dXgg.float()).all()
    for rank in range(WORLD):
        rows, og = _rows_of(rank).to(dev), _origin(rank, k0, klog)
        Xl = X[rows][:, k0:k0 + K].contiguous()
        Tl = poisoned((ML, ext), BF, dev)
        ops.lora_down_wide_drop_at(Xl, A[:, k0:k0 + K].contiguous(), n, r, rp, ext, Tl, K, P_DROP, SEED, site0, og)
        assert torch.equal(Tl, Tg[rows]), ("down", rank)
        dXl = dXg0[rows].contiguous()                                   # the local buffer keeps the logical width: the call takes a column view
        ops.lora_up_add_wide_drop_at(dXl[:, k0:k0 + K], dT[rows].contiguous(), Afull[:, k0:k0 + K], n, r, rp, K, P_DROP, SEED, site0, og)
        assert torch.equal(dXl[:, k0:k0 + K], dXg[rows][:, k0:k0 + K]), ("up_add", rank)
        assert torch.equal(dXl[:, :k0], dXg0[rows][:, :k0]) and torch.equal(dXl[:, k0 + K:], dXg0[rows][:, k0 + K:])     # nothing else written
        dXl = dXg0[rows].contiguous()
        ops.lora_up_add_wide_dgelu_drop_at(dXl[:, k0:k0 + K], dT[rows].contiguous(), Afull[:, k0:k0 + K], n, r, rp, U[rows][:, k0:k0 + K].contiguous(),
                                           K, P_DROP, SEED, site0, og)
        assert torch.equal(dXl[:, k0:k0 + K], dXgg[rows][:, k0:k0 + K]), ("dgelu", rank)
    # a rank-local key would differ: the identity map on the local rows is another mask
    Tl = poisoned((ML, ext), BF, dev)
    ops.lora_down_wide_drop(X[_rows_of(1).to(dev)].contiguous(), A, n, r, rp, ext, Tl, klog, P_DROP, SEED, site0)
    assert not torch.equal(Tl, Tg[_rows_of(1).to(dev)])


@pytest.mark.parametrize("K,k0,klog", COLS, ids=["K256", "K1024at256of1280"])
@pytest.mark.parametrize("r", [4, 24])
def test_tn_at_rank_sums_equal_the_unsharded_call(dev, r, K, k0, klog):
    """dA = dt^T (keep * x) / (1 - p) with small-integer operands and p = 0.5 (1 / (1 - p) = 2): every product, partial sum and atomic add
    is an exact integer in fp32, so the two ranks' outputs add up to the unsharded output bit for bit -- the replicated text rows' dt is
    carried by rank 0 alone, as their incoming gradient is in the engine"""
    from vt355 import ops
    gen = torch.Generator().manual_seed(7 + r + K)
    site = 9
    X = torch.randint(-3, 4, (MG, klog), generator=gen).to(BF).to(dev)
    S = torch.randint(-3, 4, (MG, r), generator=gen).to(BF).to(dev)
    full = torch.zeros(r, klog, dtype=torch.float32, device=dev)
    ops.lora_tn_wide_drop(X, S, r, full, 1, klog, 1.0, klog, 0.5, SEED, site)
    total = torch.zeros(r, K, dtype=torch.float32, device=dev)
    for rank in range(WORLD):
        rows = _rows_of(rank).to(dev)
        Sl = S[rows].clone()
        if rank != 0:
            Sl.view(2, SEGL, r)[:, NFIRST:] = 0
        part = torch.zeros(r, K, dtype=torch.float32, device=dev)
        ops.lora_tn_wide_drop_at(X[rows][:, k0:k0 + K].contiguous(), Sl, r, part, 1, K, 1.0, K, 0.5, SEED, site, _origin(rank, k0, klog))
        assert part.abs().max().item() > 0
        total += part
    assert torch.equal(total, full[:, k0:k0 + K])
    # and against numpy on the Philox mask
    keep = keep_mask(MG, klog, 0.5, SEED, site)
    ref = 2.0 * (S.double().cpu().t() @ (X.double().cpu() * keep))
    assert torch.equal(full.double().cpu(), ref)


def test_at_mask_is_the_philox_mask_of_the_unsharded_rows(dev):
    """rank 1's rows of linear2's MLP columns: dt = e_0, A = ones, dX = 0 -> dX = keep / (1 - p) exactly, so the mask itself is read back
    and compared with oracle/philox.py's at the unsharded rows and logical columns; and the down product against numpy on that mask"""
    from vt355 import ops
    K, k0, klog, site, rank = 1024, 256, 1280, 3, 1
    rows, og = _rows_of(rank), _origin(rank, k0, klog)
    keep = keep_mask(MG, klog, P_DROP, SEED, site)[rows][:, k0:k0 + K]
    dt = torch.zeros(ML, 64, dtype=BF, device=dev); dt[:, 0] = 1
    A = torch.zeros(4, K, dtype=BF, device=dev); A[0] = 1
    dX = torch.zeros(ML, K, dtype=BF, device=dev)
    ops.lora_up_add_wide_drop_at(dX, dt, A, 1, 4, 16, K, P_DROP, SEED, site, og)
    inv = torch.tensor(float(np.float32(1.0) / (np.float32(1.0) - np.float32(P_DROP))), dtype=torch.float32).to(BF).double().item()
    assert torch.equal(dX.double().cpu(), keep * inv)
    assert 0.68 < keep.mean().item() < 0.72
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(ML, K, generator=gen).to(BF)
    A4 = (torch.randn(4, K, generator=gen) * K ** -0.5).to(BF)
    T = poisoned((ML, 64), BF, dev)
    ops.lora_down_wide_drop_at(X.to(dev), A4.to(dev), 1, 4, 16, 64, T, K, P_DROP, SEED, site, og)
    ref = ((X.double() * keep) @ A4.double().t()) * float(np.float32(1.0) / (np.float32(1.0) - np.float32(P_DROP)))
    assert not bool(T[:, 4:].any())                                     # the rest of the extension is exactly zero
    err = (T[:, :4].double().cpu() - ref).abs().max().item()
    assert err <= 2.0 ** -8 * ref.abs().max().item() + 1e-6, err         # one bf16 rounding of an fp32 sum


BAD_MAPS = {"k0 % 8": (SEGL, SEGG, NFIRST, 0, 80, 4, 1280), "k0 + K > K_log": (SEGL, SEGG, NFIRST, 0, 80, 1152, 1280),
            "K_log % 4": (SEGL, SEGG, NFIRST, 0, 80, 0, 258), "seg_local <= 0": (0, SEGG, 0, 0, 80, 0, 1280),
            "seg_local < 0": (-SEGL, SEGG, 0, 0, 80, 0, 1280), "n_first > seg_local": (SEGL, SEGG, SEGL + 1, 0, 80, 0, 1280),
            "off_first < 0": (SEGL, SEGG, NFIRST, -1, 80, 0, 1280), "off_rest < 0": (SEGL, SEGG, NFIRST, 0, -80, 0, 1280),
            "e / 4 reaches 2^36 (offset)": (SEGL, SEGG, NFIRST, 0, (1 << 38) // 1280 + 1, 0, 1280),
            "e / 4 reaches 2^36 (segment)": (SEGL, 1 << 36, NFIRST, 0, 80, 0, 1280)}


@pytest.mark.parametrize("what", list(BAD_MAPS))
def test_bad_origin_maps_are_refused_before_any_launch(dev, what):
    from vt355 import ops
    from vt355._lib import VtError
    og, K = BAD_MAPS[what], 256
    X = torch.ones(ML, 1280, dtype=BF, device=dev)[:, :K]
    A, dt = torch.ones(4, K, dtype=BF, device=dev), torch.ones(ML, 64, dtype=BF, device=dev)
    T, dX = poisoned((ML, 64), BF, dev), poisoned((ML, K), BF, dev)
    out = poisoned((4, K), torch.float32, dev)
    kept = [t.clone() for t in (T, dX, out)]
    same = lambda a, b: torch.equal(a.view(torch.int16 if a.dtype == BF else torch.int32), b.view(torch.int16 if b.dtype == BF else torch.int32))
    with pytest.raises(VtError, match="bad shape"):
        ops.lora_down_wide_drop_at(X, A, 1, 4, 16, 64, T, K, P_DROP, SEED, 0, og)
    with pytest.raises(VtError, match="bad shape"):
        ops.lora_tn_wide_drop_at(X, dt, 4, out, 1, K, 1.0, K, P_DROP, SEED, 0, og)
    with pytest.raises(VtError, match="bad shape"):
        ops.lora_up_add_wide_drop_at(dX, dt, A, 1, 4, 16, K, P_DROP, SEED, 0, og)
    with pytest.raises(VtError, match="bad shape"):
        ops.lora_up_add_wide_dgelu_drop_at(dX, dt, A, 1, 4, 16, X, K, P_DROP, SEED, 0, og)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip((T, dX, out), kept))          # nothing was launched: the poison is still there
    good = (SEGL, SEGG, NFIRST, 0, 80, 0, 1280)                          # the same call with a good map runs
    ops.lora_down_wide_drop_at(X, A, 1, 4, 16, 64, T, K, P_DROP, SEED, 0, good)
    assert torch.isfinite(T.float()).all()


# ---------------------------------------------------------------------------------------------------------------- 2, 3: train steps
def _device_step(dev, r, targets, p=P_DROP, seed=SEED, train=True, **kw):
    """one training step of the tiny trunk on the device -> (model, reference_step's dict with CPU tensors)"""
    img, txt, vec, tv, cos, sin, dout = _inputs()
    m = _blocks(dev, r, targets, **({"lora_dropout": p} if p is not None else {}), **kw)
    ts = m.enable_lora_training()
    m.train(train)
    m.lora_dropout_seed = seed
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (cos.to(dev), sin.to(dev)))
    out.backward(dout.to(dev))
    grads = {n: m.lora._view(ts.grad, n).detach().float().cpu() for n in m.lora.shapes}
    return m, dict(out=out.detach().float().cpu(), dimg=xi.grad.float().cpu(), dtxt=xt.grad.float().cpu(), grads=grads,
                   raw=(out.detach().clone(), xi.grad.clone(), xt.grad.clone(), {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}))


@functools.lru_cache(maxsize=None)
def _reference(r, targets, variant, lowp):
    """the fp64 reference step (lowp: its bf16 restatement) on the adapters _blocks(., r, targets) initialises; computed once per case"""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0,
                      lora_target_modules=list(targets))
    m.load_state_dict(_oracle_weights(), strict=False)
    m.lora.init_weights(5, zero_b=False)
    base = {k: v.detach().float().double() for k, v in m.named_parameters() if not k.startswith("lora.")}
    ad = {k[5:]: v.detach().float().double() for k, v in m.named_parameters() if k.startswith("lora.")}
    return reference_step(HO, base, ad, targets, m.lora.scaling, D, M4, H, _inputs(), P_DROP, SEED, variant, BF if lowp else torch.float64)


def _check(label, got, r, targets, variant="right"):
    ok, fig = verdict(got, _reference(r, targets, variant, False), _reference(r, targets, "right", True), VALID, LI)
    print(f"[hunyuan lora dropout {label} vs {variant}] fwd {fig['fwd']:.3e}, d(img) {fig['dimg']:.3e}, d(txt) {fig['dtxt']:.3e}; adapter grads overall "
          f"{fig['overall']:.3e} (bf16 floor {fig['floor']:.3e}), worst {fig['worst']:.3e}, worst device / floor {fig['ratio']:.2f} at {fig['at']}; "
          f"bad {fig['bad'][:4]}")
    return ok, fig


@pytest.mark.parametrize("r", [4, 24, 128])
def test_all_eight_targets_dropped_train_step_matches_reference(dev, r):
    m, got = _device_step(dev, r, ALL)
    assert m.lora.wide and m.training and m.last_lora_dropout_seed == SEED and len(m.lora.shapes) == 22
    ok, fig = _check(f"all r{r}", got, r, ALL)
    assert fig["fwd"] < 1e-2 and fig["dimg"] < 3e-2 and fig["dtxt"] < 3e-2
    assert not fig["bad"], fig["bad"][:8]
    assert fig["overall"] < 1.5 * fig["floor"], (fig["overall"], fig["floor"])
    assert ok


@pytest.mark.parametrize("r,targets", [(4, FF), (24, FF), (4, ("proj_out",)), (24, ("proj_out",))], ids=["ff-r4", "ff-r24", "proj_out-r4", "proj_out-r24"])
def test_feed_forward_targets_dropped_train_step_matches_reference(dev, r, targets):
    m, got = _device_step(dev, r, targets)
    assert not m.lora.sites and len(m.lora.shapes) == 2 * len(targets)
    ok, fig = _check(f"{'+'.join(targets)} r{r}", got, r, targets)
    assert fig["fwd"] < 1e-2 and fig["dimg"] < 3e-2 and fig["dtxt"] < 3e-2
    assert not fig["bad"], fig["bad"][:8]
    assert fig["overall"] < 1.5 * fig["floor"], (fig["overall"], fig["floor"])
    assert ok


def test_device_step_fails_the_bars_against_the_wrong_variants(dev):
    """rank 24, all targets: the same device result that passes against the right masks fails against one mask per fused projection,
    the next site's masks and a missing 1 / (1 - p)"""
    m, got = _device_step(dev, 24, ALL)
    assert _check("all r24", got, 24, ALL)[0]
    for v in ("shared_qkv", "next_site", "no_scale"):
        ok, fig = _check("all r24", got, 24, ALL, v)
        assert not ok and fig["bad"], (v, fig)


# ---------------------------------------------------------------------------------------------------------------- 4: the default path
@pytest.mark.parametrize("r", [4, 24])
def test_eval_and_p0_are_the_model_without_the_argument(dev, r):
    """p = 0 (either layout) and, where the layouts agree (rank 24), model.eval() of a p = 0.3 model: output, input gradients and adapter
    gradients bit-equal to a model built without the argument.  B 1, 40 + 8 rows: the rank-gradient kernel's row slices add with fp32
    atomics in arrival order, and only a single slice (at most 64 rows) makes its sums reproducible to the bit."""
    from vt355.hunyuan import HunyuanBlocks
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs(21, 1, 40, 8)]

    def run(eval_mode=False, **kw):
        m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0,
                          lora_target_modules=list(ALL), **kw)
        m.load_state_dict(_oracle_weights(), strict=False)
        m.lora.init_weights(5, zero_b=False)
        m.to(dev)
        ts = m.enable_lora_training()
        if eval_mode:
            m.eval()
        xi, xt = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        out = m(xi, xt, vec, tv, (cos, sin))
        out.backward(dout)
        return m, out.detach().clone(), xi.grad.clone(), xt.grad.clone(), ts.grad.detach().clone()
    ref = run()
    assert ref[0].lora.wide == (r > 21) and torch.isfinite(ref[1].float()).all() and ref[4].abs().max().item() > 0
    cases = [("p0", run(lora_dropout=0.0))]
    if r > 21:
        cases.append(("eval", run(eval_mode=True, lora_dropout=P_DROP)))
    for label, got in cases:
        assert got[0].lora.wide == ref[0].lora.wide and got[0].last_lora_dropout_seed is None, label
        for i, what in ((1, "out"), (2, "d(img)"), (3, "d(txt)"), (4, "adapter gradients")):
            assert torch.equal(got[i], ref[i]), (label, what)
    # in training mode the same p = 0.3 model does drop
    m = run(lora_dropout=P_DROP)
    assert m[0].last_lora_dropout_seed is not None and not torch.equal(m[1], ref[1])


def test_eval_at_rank_4_runs_the_wide_undropped_launches(dev, monkeypatch):
    """rank 4 with p > 0 is the wide layout (there is nowhere to mask in the narrow one): its eval() forward is bit-equal to the model
    without the argument in that layout (VT355_LORA_WIDE=1)"""
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    m = _blocks(dev, 4, ALL, lora_dropout=P_DROP)
    m.eval()
    with torch.no_grad():
        o1 = m(img, txt, vec, tv, (cos, sin))
    monkeypatch.setenv("VT355_LORA_WIDE", "1")
    m0 = _blocks(dev, 4, ALL)
    assert m0.lora.wide
    with torch.no_grad():
        o0 = m0(img, txt, vec, tv, (cos, sin))
    assert torch.isfinite(o1.float()).all() and torch.equal(o1, o0) and m.last_lora_dropout_seed is None


# ---------------------------------------------------------------------------------------------------------------- 5: seeds
def test_seeds(dev):
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    m = _blocks(dev, 24, ALL, lora_dropout=P_DROP)
    f = lambda: m(img, txt, vec, tv, (cos, sin))
    with torch.no_grad():
        m.lora_dropout_seed = 11
        a, b = f(), f()
        assert m.last_lora_dropout_seed == 11 and torch.isfinite(a.float()).all() and torch.equal(a, b)
        m.lora_dropout_seed = 12
        c = f()
        assert m.last_lora_dropout_seed == 12 and not torch.equal(a, c)
        m.lora_dropout_seed = None
        d = f(); s1 = m.last_lora_dropout_seed
        e = f(); s2 = m.last_lora_dropout_seed
        assert s1 is not None and s2 is not None and s1 != s2 and not torch.equal(d, e)
        m.lora_dropout_seed = s1                                        # the recorded seed reproduces its forward
        assert torch.equal(f(), d)
        m.eval()
        m.lora_dropout_seed = None
        g = f()
        assert torch.equal(g, f()) and not torch.equal(g, a)


# ---------------------------------------------------------------------------------------------------------------- 6: the fp8 modes
def test_fp8_weights_mode_dropped_is_the_bf16_model_on_dequantised_weights(dev):
    """test_fp8_weights_mode_is_the_bf16_model_on_dequantised_weights with p = 0.3: same output bits, adapter gradients within 1e-4 (the
    rank-gradient kernel's fp32 atomics)"""
    from vt355 import ops
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    mq = _blocks(dev, 24, ALL, fp8="weights", lora_dropout=P_DROP)
    mb = _blocks(dev, 24, ALL, lora_dropout=P_DROP)
    sd = {}
    for k, v in mq.state_dict().items():
        if k in mq.shapes and k.endswith(".weight") and len(mq.shapes[k]) == 2:
            wq, sw = ops.quantize_fp8(v.to(dev, BF).contiguous())
            v = (wq.float() * sw).to(BF)
        sd[k] = v
    mb.load_state_dict(sd, strict=True)
    mb.to(dev)
    outs, grads = [], []
    for m in (mq, mb):
        ts = m.enable_lora_training()
        m.lora_dropout_seed = SEED
        o = m(img, txt, vec, tv, (cos, sin))
        o.backward(dout)
        assert m.last_lora_dropout_seed == SEED
        outs.append(o.detach().clone())
        grads.append({n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes})
    mb.eval()
    with torch.no_grad():
        o_eval = mb(img, txt, vec, tv, (cos, sin))
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], o_eval)
    for n in grads[0]:
        assert grads[1][n].abs().max().item() > 0 and rel_l2(grads[0][n], grads[1][n]) < 1e-4, n


def _fp8_dropped(dev, mode):
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8=mode, lora_rank=24, lora_alpha=2.0,
                      lora_target_modules=list(ALL), lora_dropout=P_DROP).to(dev).init_weights(4)
    m.lora.init_weights(5, zero_b=False)
    with torch.no_grad():
        for n, p in m.lora._plist.items():
            if ".lora_B" in n:
                p.mul_(10.0)
    m.lora_dropout_seed = SEED
    return m, m.enable_lora_training()


def test_fp8_matmul_and_mfma_dropped_against_weights_mode(dev):
    """_fp8_blocks' model (2 + 2 blocks, B x 10) with p = 0.3, seed pinned.  "matmul" against "weights": the image rows within
    test_fp8_matmul_mode_with_all_targets' 8e-2, every adapter gradient finite and non-zero.  "mfma" against "weights":
    test_fp8_mfma_against_weights_mode's bars -- the adapters' contribution out(B) - out(B = 0) within 0.25, every adapter gradient
    within 8e-2 (the forward tail is unchanged, t comes from the masked input)"""
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    res = {}
    for mode in ("weights", "matmul", "mfma"):
        m, ts = _fp8_dropped(dev, mode)
        with torch.no_grad():
            m(img, txt, vec, tv, (cos, sin))                  # mfma: seeds the history, the runs below all use delayed scales
            o_b = m(img, txt, vec, tv, (cos, sin)).float()
            saved = {n: p.detach().clone() for n, p in m.lora._plist.items() if ".lora_B" in n}
            for n in saved:
                m.lora._plist[n].zero_()
            m.lora._packed = None
            o_0 = m(img, txt, vec, tv, (cos, sin)).float()
            for n, v in saved.items():
                m.lora._plist[n].copy_(v)
            m.lora._packed = None
        out = m(img, txt, vec, tv, (cos, sin))
        out.backward(dout)
        assert m.training and m.last_lora_dropout_seed == SEED and torch.isfinite(ts.grad).all()
        res[mode] = (o_b - o_0, {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}, o_b, out.detach()[:, :LI].float())
    for n, g in res["matmul"][1].items():
        assert g.abs().max().item() > 0, n
    e = rel_l2(res["matmul"][3], res["weights"][3])
    contrib = rel_l2(res["mfma"][0], res["weights"][0])
    errs = sorted(((rel_l2(res["mfma"][1][n], res["weights"][1][n]), n) for n in res["weights"][1]), reverse=True)
    print(f"[hunyuan lora dropout fp8] matmul image rows vs weights rel-L2 {e:.3e}; mfma adapter contribution vs weights {contrib:.3e}; "
          f"|contribution| {res['weights'][0].norm().item():.3e} of |out| {res['weights'][2].norm().item():.3e}; worst adapter gradients "
          f"{[(n, f'{a:.2e}') for a, n in errs[:4]]}")
    assert 0 < e < 8e-2
    assert len(errs) == 2 * 22
    assert res["weights"][0].norm().item() > 0.05 * res["weights"][2].norm().item()
    assert contrib < 0.25 and errs[0][0] < 8e-2


# ---------------------------------------------------------------------------------------------------------------- 7: the whole model
def test_whole_model_flow_training_step_with_dropout(dev):
    """HunyuanVideoFlow.training_step with all targets and p = 0.3: finite loss, every adapter gradient non-zero, a seed drawn and
    recorded -- and pinning the recorded seed reproduces the step (loss and gradients up to the fp32 atomics of the loss reduction and
    the rank-gradient kernel: 1e-6 / 1e-4), another seed does not"""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanVideoFlow, HYVideoDiffusionTransformer
    m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=24, lora_alpha=2.0, lora_target_modules=list(ALL),
                                    lora_dropout=P_DROP)
    m.load_state_dict(HO.init_model(HO.model_shapes(256, 2, 1, 1, 4, 4, (1, 2, 2), 64, 32), 3), strict=False)
    m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    flow = HunyuanVideoFlow(model=m, learning_rate=1e-3).to(dev)
    flow.configure_optimizers()
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k]).to(dev)
    batch = {"latents": T("x"), "prompt_embeds": T("text_states"), "prompt_attention_mask": T("text_mask"), "pooled_prompt_embeds": T("text_states_2")}
    ts = m.lora.train_state

    def step(seed):
        m.lora_dropout_seed = seed
        ts.grad.zero_()
        torch.manual_seed(0)
        loss = flow.training_step(batch)
        loss.backward()
        return loss.detach().clone(), ts.grad.detach().clone(), m.last_lora_dropout_seed
    l1, g1, s1 = step(None)
    assert s1 is not None and m.lora_dropout_seed is None
    assert torch.isfinite(l1) and torch.isfinite(g1).all() and len(m.lora.shapes) == 22
    for n in m.lora.shapes:
        assert m.lora._view(g1, n).abs().max().item() > 0, n
    l2, g2, s2 = step(s1)
    assert s2 == s1 and abs(l2.item() - l1.item()) <= 1e-6 * abs(l1.item()) and rel_l2(g2, g1) < 1e-4
    l3, g3, s3 = step(s1 + 1)
    assert s3 == s1 + 1 and rel_l2(g3, g1) > 1e-2
    m.eval()
    le, ge, se = step(None)
    assert se == s3 and rel_l2(ge, g1) > 1e-2                            # eval: nothing drawn, nothing dropped


# ---------------------------------------------------------------------------------------------------------------- 8: sequence parallelism
def _sp_worker(rank, world, port, res):
    """test_hunyuan_lora_ff_gpu._sp_worker's run (2 + 2 blocks, rank 4, all eight targets) with p = 0.3 and the seed pinned; rank 0 also
    holds the unsharded run against the fp64 reference with the right masks and with masks keyed by the rank-local row"""
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("VT355_LORA_WIDE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import hunyuan_oracle as HO
        import vt355.hunyuan as hy
        _poison_engine(setattr)
        dev = torch.device("cuda:0")
        b, Li, Lt = 2, 96, 12
        m = hy.HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=2, mm_single_blocks_depth=2, lora_rank=4, lora_alpha=2.0,
                             lora_target_modules=list(ALL), lora_dropout=P_DROP)
        m.init_weights(3)
        m.lora.init_weights(5, zero_b=False)
        base = {k: v.detach().float().double() for k, v in m.named_parameters() if not k.startswith("lora.")}
        ad = {k[5:]: v.detach().float().double() for k, v in m.named_parameters() if k.startswith("lora.")}
        m.to(dev)
        ts = m.enable_lora_training()
        g = torch.Generator().manual_seed(17)
        img, txt, vec = (torch.randn(b, Li, D, generator=g) * 0.5).to(BF), (torch.randn(b, Lt, D, generator=g) * 0.5).to(BF), torch.randn(b, D, generator=g).to(BF)
        ang = torch.rand(Li, 64, generator=g) * 6.28
        cos, sin = torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()
        tv = torch.tensor([12, 7])
        gout = (torch.randn(b, Li + Lt, D, generator=g) * 0.1).to(BF)
        gout[1, Li + 7:] = 0                                                        # padding text rows carry no gradient

        def run(sl, group):
            m.set_sequence_parallel(group)
            m.lora_dropout_seed = SEED
            ts.grad.zero_()
            xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img[:, sl], txt, vec)]
            out = m(xi, xt, xv, tv.to(dev), (cos[sl].to(dev), sin[sl].to(dev)))
            go = torch.cat([gout[:, sl], gout[:, Li:]], 1) if group is not None else gout
            if group is not None:                                                   # the text rows' incoming gradient arrives ONCE in total: rank 0 carries it
                go = go.clone()
                if rank != 0:
                    go[:, sl.stop - sl.start:] = 0
            out.backward(go.to(dev))
            torch.cuda.synchronize()
            return out.detach().float().cpu(), xi.grad.float().cpu(), xt.grad.float().cpu(), xv.grad.float().cpu(), ts.grad.detach().clone()

        full = run(slice(0, Li), None)
        n = Li // world
        sl = slice(rank * n, (rank + 1) * n)
        part = run(sl, dist.group.WORLD)
        # a direct training-mode forward under sequence parallelism without a pinned seed is refused (before any communication)
        m.lora_dropout_seed = None
        try:
            m(img[:, sl].to(dev), txt.to(dev), vec.to(dev), tv.to(dev), (cos[sl].to(dev), sin[sl].to(dev)))
            refused = 0.0
        except RuntimeError as ex:
            refused = 1.0 if "lora_dropout_seed" in str(ex) else 0.0
        m.set_sequence_parallel(None)
        valid = torch.ones(b, Lt, 1); valid[1, 7:] = 0
        errs = {"out_img": rel_l2(part[0][:, :n], full[0][:, sl]), "out_txt": rel_l2(part[0][:, n:] * valid, full[0][:, Li:] * valid),
                "dimg": rel_l2(part[1], full[1][:, sl])}
        for name, idx in (("dtxt", 2), ("dvec", 3)):
            tot = part[idx].to(dev); dist.all_reduce(tot)
            errs[name] = rel_l2(tot.cpu() * (valid if idx == 2 else 1), full[idx] * (valid if idx == 2 else 1))
        gsum = part[4].clone(); dist.all_reduce(gsum)
        errs["params"] = rel_l2(gsum, full[4])
        rels = []                                                                   # parity.rel_l2 refuses non-finite input
        for name in m.lora.shapes:
            a, b_ = m.lora._view(gsum, name), m.lora._view(full[4], name)
            if b_.norm().item() > 0:
                rels.append(rel_l2(a, b_))
        errs["worst_param"] = sorted(rels)[-1]
        errs["zero_grads"] = float(len(m.lora.shapes) - len(rels))
        errs["refused"] = refused
        if rank == 0:                   # the unsharded device run against the reference keyed by unsharded rows / by rank-local rows
            for variant in ("right", "local_rows"):
                ref = reference_step(HO, base, ad, ALL, m.lora.scaling, D, M4, H, (img, txt, vec, tv, cos, sin, gout), P_DROP, SEED, variant,
                                     world=world, n_double=2, n_single=2)
                flat = torch.cat([ref["grads"][k].flatten() for k in m.lora.shapes])
                errs[f"ref_{variant}_params"] = rel_l2(torch.cat([m.lora._view(full[4], k).flatten() for k in m.lora.shapes]).double().cpu(), flat)
                errs[f"ref_{variant}_dimg"] = rel_l2(full[1], ref["dimg"])
        res[rank] = errs
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_dropped_run_under_ulysses_world2_matches_unsharded(dev):
    """two ranks with the seed pinned equal the unsharded dropped run under test_all_targets_under_ulysses_world2_match_unsharded's bars
    (1e-2; 5e-2 for the worst single adapter gradient): the masks are keyed by the unsharded row.  The unsharded run itself is the
    reference's with those masks (adapter gradients within that test's loosest bar, 5e-2, of the fp64 reference) and is NOT the
    reference's with masks keyed by the rank-local row"""
    import torch.multiprocessing as mp
    from test_hunyuan_sp_gpu import _free_port
    mgr = mp.Manager(); res = mgr.dict()
    mp.spawn(_sp_worker, args=(2, _free_port(), res), nprocs=2, join=True)
    for r in (0, 1):
        print(f"[hunyuan sp-2 lora dropout] rank {r}: " + ", ".join(f"{k} {v:.2e}" for k, v in res[r].items()))
    for r in (0, 1):
        errs = dict(res[r])
        assert errs.pop("zero_grads") == 0 and errs.pop("refused") == 1.0
        refs = {k: errs.pop(k) for k in list(errs) if k.startswith("ref_")}
        for k, v in errs.items():
            assert v < (5e-2 if k == "worst_param" else 1e-2), (r, k, v)
        if r == 0:
            assert refs["ref_right_params"] < 5e-2 and refs["ref_right_dimg"] < 3e-2, refs
            assert refs["ref_local_rows_params"] > 5e-2, refs
