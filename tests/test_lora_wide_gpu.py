"""LoRA ranks 17..128 for the CogVideoX DiT on the GPU: the MFMA rank-side kernels of csrc/lora_wide.hip against fp32 host products
of the bf16-rounded operands (so only the output's bf16 rounding and the fp32 summation order are left as error; the bars are
those of test_kernels_gpu.py::test_lora_kernels), and the tiny training step against the fp64 oracle under the project's own bars.

The rank-gradient kernel sums its row slices with fp32 atomics only (it has no two-stage mode), so no bitwise-repeatability
assertion is made for it."""
import pytest
import torch

from parity import close, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rb(x):      # bf16-round but keep fp32 (what the device kernel actually sees)
    return x.to(BF).float()


def layout(n, r):
    rp = (r + 15) // 16 * 16
    return rp, (n * rp + 63) // 64 * 64


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("r", [17, 32, 128])
@pytest.mark.parametrize("n", [3, 1])
@pytest.mark.parametrize("K", [128, 192])
def test_down_wide(dev, K, n, r):
    """every adapter of a projection in one pass: 200 rows = three full 64-row blocks and a tail of 8 (a partial 16-row tile); the NaN
    pre-fill shows every extension column is written, padding and tail as exact zeros; the base columns are not touched"""
    from vt355 import ops
    g = torch.Generator().manual_seed(100 * K + 10 * n + r)
    M = 200
    rp, ext = layout(n, r)
    x = rb(torch.randn(M, K, generator=g)); A = rb(torch.randn(n * r, K, generator=g) * 0.1)
    X = torch.full((M, K + ext), float("nan"), dtype=BF, device=dev); X[:, :K] = x.to(dev, BF)
    ops.lora_down_wide(X, A.to(dev, BF), n, r, rp, ext, X[:, K:], K)
    T = X[:, K:].float().cpu()
    pad = torch.ones(ext, dtype=torch.bool)
    for j in range(n):
        close(T[:, j * rp:j * rp + r], x @ A[j * r:(j + 1) * r].T, 1e-2, 1e-2, f"down_wide adapter {j}")
        pad[j * rp:j * rp + r] = False
    assert pad.sum().item() == ext - n * r
    assert torch.equal(T[:, pad], torch.zeros(M, int(pad.sum())))          # exactly 0.0 (NaN would fail too)
    assert torch.equal(X[:, :K].cpu(), x.to(BF))


@pytest.mark.parametrize("R", [17, 64, 128])
@pytest.mark.parametrize("orient", ["osr1", "osp1"])
def test_rank_gradients_wide(dev, R, orient):
    """out[p*osp + i*osr] += alpha * sum_m Big[m,p] Small[m,i]: 1100 rows = 18 row tiles of 64 (more than one slice) with a tail of 12,
    P = 192 = one full 128-column block and half of one; both output orientations (dB: osr == 1, dA: osp == 1); operands are strided
    views as in the engine; accumulates onto a non-zero out"""
    from vt355 import ops
    g = torch.Generator().manual_seed(7 * R + len(orient))
    M, P, alpha = 1100, 192, 0.25
    big = rb(torch.randn(M, P + 64, generator=g)); small = rb(torch.randn(M, 16 + R + 5, generator=g))
    ref = alpha * big[:, :P].T @ small[:, 16:16 + R]                          # [P, R]
    start = torch.randn(P, R, generator=g)
    bd, sd = big.to(dev, BF), small.to(dev, BF)
    if orient == "osr1":
        out = start.clone().to(dev)
        ops.lora_tn_wide(bd, sd[:, 16:], R, out, R, 1, alpha, P)
        close(out, start + ref, 1e-3, 1e-2, f"tn_wide R={R} osr=1")
    else:
        out = start.T.contiguous().to(dev)                                  # [R, P]
        ops.lora_tn_wide(bd, sd[:, 16:], R, out, 1, P, alpha, P)
        close(out, (start + ref).T, 1e-3, 1e-2, f"tn_wide R={R} osp=1")


def test_rank_gradients_wide_several_tiles_per_slice(dev):
    """40 012 rows = 626 row tiles: more than the slice count, so every block walks several 64-row tiles (re-staging its LDS blocks)
    before it adds its partial sums; the last slice ends on a tile of 12 rows"""
    from vt355 import ops
    g = torch.Generator().manual_seed(11)
    M, P, R, alpha = 40012, 192, 64, 0.25
    big = rb(torch.randn(M, P, generator=g)); small = rb(torch.randn(M, R, generator=g))
    ref = (alpha * big.double().T @ small.double()).float()
    out = torch.full((P, R), 2.0, device=dev)
    ops.lora_tn_wide(big.to(dev, BF), small.to(dev, BF), R, out, R, 1, alpha, P)
    close(out, 2.0 + ref, 1e-3, 1e-2, "tn_wide long M")


@pytest.mark.parametrize("r", [17, 128])
def test_up_add_wide(dev, r):
    """dX += sum_j dT_j A_j in place, three adapters at once; dT is the extension of the same buffer (as in the engine): only [:, :K] changes"""
    from vt355 import ops
    g = torch.Generator().manual_seed(r)
    M, K, n = 200, 192, 3
    rp, ext = layout(n, r)
    dx = rb(torch.randn(M, K, generator=g)); A = rb(torch.randn(n * r, K, generator=g) * 0.1)
    dT = torch.zeros(M, ext)
    ref = dx.clone()
    for j in range(n):
        dT[:, j * rp:j * rp + r] = rb(torch.randn(M, r, generator=g))
        ref += dT[:, j * rp:j * rp + r] @ A[j * r:(j + 1) * r]
    DX = torch.cat([dx, dT], 1).to(dev, BF)
    before = DX.clone()
    ops.lora_up_add_wide(DX, DX[:, K:], A.to(dev, BF), n, r, rp, K)
    close(DX[:, :K], ref, 1e-2, 2e-2, "up_add_wide")
    assert torch.equal(DX[:, K:], before[:, K:])
    assert not torch.equal(DX[:, :K], before[:, :K])


@pytest.mark.parametrize("r", [17, 128])
def test_pack_wide(dev, r):
    from vt355 import ops
    g = torch.Generator().manual_seed(50 + r)
    n, N, K = 3, 256, 128
    rp, ext = layout(n, r)
    Bc = torch.randn(n * N, r, generator=g)
    ref = torch.zeros(n * N, ext)
    for j in range(n):
        ref[j * N:(j + 1) * N, j * rp:j * rp + r] = 0.25 * Bc[j * N:(j + 1) * N]
    outside = ref == 0
    W = torch.full((n * N, K + ext), 7.0, dtype=BF, device=dev)
    ops.lora_pack_b_wide(Bc.to(dev), W[:, K:], K + ext, n, N, r, rp, ext, 0.25)
    close(W[:, K:], ref, 1e-2, 1e-3, "pack_b_wide"); assert (W[:, :K] == 7).all()
    assert (W[:, K:].float().cpu()[outside] == 0).all()
    WT = torch.full((K + ext, n * N), 7.0, dtype=BF, device=dev)
    ops.lora_pack_bt_wide(Bc.to(dev), WT[K:], n * N, n, N, r, rp, ext, 0.25)
    close(WT[K:], ref.T, 1e-2, 1e-3, "pack_bt_wide"); assert (WT[:K] == 7).all()
    assert (WT[K:].float().cpu()[outside.T] == 0).all()


def test_wide_entry_points_refuse_bad_shapes(dev):
    from vt355 import ops
    from vt355._lib import VtError
    x = torch.zeros(64, 128 + 64, dtype=BF, device=dev); a = torch.zeros(3 * 129, 128, dtype=BF, device=dev)
    with pytest.raises(VtError):
        ops.lora_down_wide(x, a, 3, 129, 144, 448, x[:, 128:], 128)           # rank above 128
    with pytest.raises(VtError):
        ops.lora_down_wide(x, a, 1, 17, 24, 64, x[:, 128:], 128)              # column stride not a multiple of 16
    with pytest.raises(VtError):
        ops.lora_tn_wide(x, x[:, 128:], 129, torch.zeros(128, 129, device=dev), 129, 1, 1.0, 128)
    with pytest.raises(VtError):
        ops.lora_up_add_wide(x, x[:, 128:], a, 1, 17, 32, 100)                # K not a multiple of 64


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("r,rope", [(17, False), (32, False), (64, False), (128, False), (32, True)])
def test_tiny_train_step_wide_ranks(dev, r, rope, monkeypatch):
    """forward, loss and LoRA gradients of one tiny training step against the fp64 oracle, under the bars the project keeps for r <= 16"""
    from selfcheck import tiny_train_step_check
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    res = tiny_train_step_check(B=2, lora_r=r, rope=rope)
    print(f"r={r} rope={rope}: {res}")


def test_tiny_train_step_rank16_forced_wide(dev, monkeypatch):
    """VT355_LORA_WIDE=1 puts the wide kernels at a rank the narrow path also covers: same bars"""
    from selfcheck import build_tiny, tiny_train_step_check
    monkeypatch.setenv("VT355_LORA_WIDE", "1")
    assert build_tiny(dev, lora_r=16)[3].wide
    res = tiny_train_step_check(B=2, lora_r=16)
    print(f"r=16 forced wide: {res}")


def test_block_recompute_gives_the_same_gradients_rank32(dev):
    """test_model_gpu.py::test_block_recompute_gives_the_same_gradients[lora] at rank 32: same loss bit for bit, same gradients up to
    the order of the fp32 atomic adds"""
    from vt355.scheduler import CogVideoXDPMScheduler
    from vt355.workflow import _LossFn
    from selfcheck import build_tiny
    cfg, model, peft, st = build_tiny(dev, lora_r=32)
    assert st.wide and st.ext_qkv == 128
    g = torch.Generator().manual_seed(3)
    Fr = (cfg.sample_frames - 1) // 4 + 1
    x0 = torch.randn(2, Fr, 16, cfg.sample_height, cfg.sample_width, generator=g).to(dev)
    text = (torch.randn(2, cfg.max_text_seq_length, cfg.text_embed_dim, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    t = torch.tensor([120, 870], device=dev)
    sched = CogVideoXDPMScheduler()
    noisy = sched.add_noise(x0, torch.randn(x0.shape, generator=g).to(dev), t)
    sa, sb, w = sched.coefficients(t)

    def step(policy):
        model.enable_gradient_checkpointing(policy)
        st.grad.zero_()
        out = peft(hidden_states=noisy, encoder_hidden_states=text, timestep=t)[0]
        loss = _LossFn.apply(out, noisy, x0, sa, sb, w)
        loss.backward()
        return loss.item(), st.grad.clone()
    l0, g0 = step("never")
    l1, g1 = step("always")
    assert l0 == l1
    assert g0.abs().max().item() > 0
    rel = rel_l2(g1, g0)
    assert rel < 1e-3, rel


def test_lora_checkpoint_round_trip_rank32(dev, tmp_path):
    from types import SimpleNamespace
    from vt355 import checkpoint as C
    from vt355.workflow import CogVideoXWorkFlow
    from selfcheck import build_tiny
    _, _, src, _ = build_tiny(dev, lora_r=32, seed=0)
    with torch.no_grad():
        for n, p in src.named_parameters():
            if "lora_B" in n:
                p.fill_(0.375)
    src._lora_state.mark_changed()
    wf = SimpleNamespace(model=src, global_step=5)
    wf.on_save_checkpoint = lambda ck: CogVideoXWorkFlow.on_save_checkpoint(wf, ck)
    path = C.save_checkpoint(wf, str(tmp_path / "checkpoints" / "last.ckpt"))
    sd = C.load_checkpoint_file(path)["state_dict"]
    assert len(sd) == 2 * 4 * 2 and all("lora" in k for k in sd)
    d = src.inner_dim
    assert all(tuple(v.shape) == ((32, d) if "lora_A" in k else (d, 32)) for k, v in sd.items())
    _, _, dst, st = build_tiny(dev, lora_r=32, seed=1)
    assert C.load_lora_from_ckpt(dst, path) == 16
    for (n, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        if "lora" in n:
            assert torch.equal(a, b), n
        if "lora_B" in n:
            assert (b == 0.375).all()
    assert (st.b_qkv(st.flat_bf16, 1) == 0.375).all()          # the compute copy followed the load
