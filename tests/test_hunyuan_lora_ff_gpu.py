"""HunyuanVideo LoRA feed-forward targets on the device (lora_target_modules: ff.net.0.proj -> img_mlp.fc1, ff.net.2 -> img_mlp.fc2,
proj_mlp -> the MLP rows of linear1, proj_out -> linear2): train steps against the fp64 oracle on the effective weights W + scaling B A
(tests/hunyuan_lora_ff_ref.py) in both K-extension layouts, the fp8 modes, repacking, partial backward, the whole model and Ulysses
sequence parallelism.  Tiny trunk: D 256, 2 heads of 128, 4D = 1024, D + 4D = 1280; 1 double + 1 single block; B 2, 160 image + 32 text
rows with valid text lengths 32 and 19.  Every activation / gradient buffer the engine allocates starts out poisoned (parity.poisoned), so
an extension column or an output element that no kernel wrote shows as NaN."""
import functools
import os

import numpy as np
import pytest
import torch

from hunyuan_lora_ff_ref import ALL, ATTN, FF, blocks_loss, lora_effective
from parity import bf16_leaves, cosine, floor_report, poisoned, rel_l2

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D, H, M4 = 256, 2, 1024
B, LI, LT, VALID = 2, 160, 32, (32, 19)


def _poison_engine(setattr_):
    from vt355.hunyuan import _HYRun
    setattr_(_HYRun, "E", lambda self, *s, dt=BF: poisoned(tuple(s), dt, self.dev))


@pytest.fixture(autouse=True)
def _poisoned_buffers(monkeypatch):
    monkeypatch.delenv("VT355_LORA_WIDE", raising=False)
    _poison_engine(monkeypatch.setattr)


@functools.lru_cache(maxsize=None)
def _inputs(seed=31, b=B, li=LI, lt=LT):
    """CPU tensors: img, txt, vec, valid text lengths, cos, sin, the output gradient (zero on padding text rows)"""
    gen = torch.Generator().manual_seed(seed)
    img, txt, vec = torch.randn(b, li, D, generator=gen).to(BF), torch.randn(b, lt, D, generator=gen).to(BF), torch.randn(b, D, generator=gen).to(BF)
    ang = torch.rand(li, 64, generator=gen) * 6.28
    cos, sin = torch.repeat_interleave(ang.cos(), 2, dim=1).contiguous(), torch.repeat_interleave(ang.sin(), 2, dim=1).contiguous()
    tv = torch.tensor([min(v, lt) for v in VALID[:b]])
    dout = torch.randn(b, li + lt, D, generator=gen).to(BF)
    for i in range(b):
        dout[i, li + int(tv[i]):] = 0
    return img, txt, vec, tv, cos, sin, dout


@functools.lru_cache(maxsize=None)
def _oracle_weights():
    import hunyuan_oracle as HO
    return {**HO.init(HO.double_block_shapes(D, H, pre="double_blocks.0."), 1), **HO.init(HO.single_block_shapes(D, H, pre="single_blocks.0."), 2)}


def _blocks(dev, r, targets, seed=5, **kw):
    """one double + one single block with the oracle's weights and adapters of rank r on `targets` (zero_b=False)"""
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=1, mm_single_blocks_depth=1, lora_rank=r, lora_alpha=2.0,
                      lora_target_modules=None if targets is None else list(targets), **kw)
    m.load_state_dict(_oracle_weights(), strict=False)
    m.lora.init_weights(seed, zero_b=False)
    return m.to(dev)


def _train_step_vs_oracle(dev, r, targets, label):
    """forward 1e-2 of scale, input gradients 3e-2, every adapter gradient under parity.floor_bars from the bf16 restatement (cosine 0.98,
    cap 0.2), overall under 1.5 x the restatement's own overall figure: test_wide_lora_blocks_train_step_matches_oracle's bars.  No
    parameter has a margin of its own."""
    import hunyuan_oracle as HO
    img, txt, vec, tv, cos, sin, dout = _inputs()
    m = _blocks(dev, r, targets)
    ts = m.enable_lora_training()
    assert m.train_state is None and ts.numel == m.lora.numel
    xi, xt, xv = [t.to(dev).requires_grad_(True) for t in (img, txt, vec)]
    out = m(xi, xt, xv, tv.to(dev), (cos.to(dev), sin.to(dev)))
    out.backward(dout.to(dev))
    base = {k: v.detach().float().cpu().double() for k, v in m.named_parameters() if not k.startswith("lora.")}
    ad = {k[5:]: v.detach().float().cpu().double().requires_grad_(True) for k, v in m.named_parameters() if k.startswith("lora.")}
    assert set(ad) == set(m.lora.shapes)
    s = m.lora.scaling
    ri, rt, rv = [t.double().requires_grad_(True) for t in (img, txt, vec)]
    xo, loss = blocks_loss(HO, lora_effective(base, ad, targets, s, D, M4), ri, rt, rv, tv, cos.double(), sin.double(), dout, H)
    loss.backward()
    vm = torch.zeros(B, LI + LT, 1, dtype=torch.float64)
    for i in range(B):
        vm[i, :LI + int(tv[i])] = 1
    tm = vm[:, LI:]
    e = rel_l2(out.double().cpu() * vm, xo * vm)
    ei, et = rel_l2(xi.grad, ri.grad), rel_l2(xt.grad.double().cpu() * tm, rt.grad * tm)
    adb = bf16_leaves(ad)
    bl = lambda t: t.detach().to(BF).requires_grad_(True)
    bo, bloss = blocks_loss(HO, lora_effective({k: v.to(BF) for k, v in base.items()}, adb, targets, s, D, M4), bl(img), bl(txt), bl(vec), tv,
                            cos, sin, dout, H)
    assert bo.dtype == BF
    bloss.backward()
    overall, ofloor, worst, bad, ratio, at = floor_report([(n, m.lora._view(ts.grad, n), ad[n].grad) for n in m.lora.shapes],
                                                          {n: adb[n].grad for n in m.lora.shapes}, 0.98, 0.2)
    print(f"[hunyuan lora ff {label}] fwd rel-L2 {e:.3e}, d(img) {ei:.3e}, d(txt) {et:.3e}; {len(ad)} adapter grads overall rel-L2 {overall:.3e} "
          f"(bf16 floor {ofloor:.3e}), worst {worst:.3e}, worst device / floor {ratio:.2f} at {at}")
    assert e < 1e-2
    assert ei < 3e-2 and et < 3e-2
    assert not bad, bad[:8]
    assert overall < 1.5 * ofloor, (overall, ofloor)
    return m


# ---------------------------------------------------------------------------------------------------------------- 1, 2: against the oracle
@pytest.mark.parametrize("r", [4, 24, 128])
def test_all_eight_targets_train_step_matches_oracle(dev, r):
    """rank 4: the narrow layout (three adapters side by side in 64 columns); 24: the wide one, rp 32; 128: four adapters of 128 rank columns
    on linear1's input, more than one 384-column tail holds -- the MLP adapter's extension lies in front of x and is its product's own tail"""
    m = _train_step_vs_oracle(dev, r, ALL, f"all r{r}")
    assert m.lora.wide == (r > 21) and len(m.lora.shapes) == 22 and m.lora.ext_ff == (64 if r <= 64 else 128)


@pytest.mark.parametrize("r,targets", [(24, FF), (4, FF), (4, ("proj_out",)), (24, ("proj_out",))],
                         ids=["ff-r24", "ff-r4", "proj_out-r4", "proj_out-r24"])
def test_feed_forward_targets_without_the_attention_group(dev, r, targets):
    """the four feed-forward targets alone, and proj_out alone: the same bars; adapters that were not requested do not exist"""
    m = _train_step_vs_oracle(dev, r, targets, f"{'+'.join(targets)} r{r}")
    assert not m.lora.sites and len(m.lora.shapes) == 2 * len(targets)
    assert all(".img_attn_" not in n and ".lora_A.q." not in n for n in m.lora.shapes)
    if targets == ("proj_out",):
        assert list(m.lora.shapes) == ["single_blocks.0.linear2.lora_A.weight", "single_blocks.0.linear2.lora_B.weight"]


# ---------------------------------------------------------------------------------------------------------------- 3: the fp8 modes
def test_fp8_weights_mode_is_the_bf16_model_on_dequantised_weights(dev):
    """fp8="weights" at rank 24, all targets: the extended operands' base columns are the de-quantised E4M3 weights, so a bf16 model loaded
    with those (and the same adapters) gives the same output and the same adapter gradients bit for bit -- up to the fp32 atomics of the
    rank-gradient kernel, whose sums depend on arrival order (1e-4, as test_partial_backward_touches_only_the_adapters_it_reaches)"""
    from vt355 import ops
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    mq = _blocks(dev, 24, ALL, fp8="weights")
    mb = _blocks(dev, 24, ALL)
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
        o = m(img, txt, vec, tv, (cos, sin))
        o.backward(dout)
        outs.append(o.detach().clone())
        grads.append({n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes})
    with torch.no_grad():
        for p in mb.lora._plist.values():
            p.zero_()
        mb.lora._packed = None
        o0 = mb(img, txt, vec, tv, (cos, sin))
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])
    assert not torch.equal(o0, outs[1])                              # the adapters contribute
    for n in grads[0]:
        assert grads[1][n].abs().max().item() > 0 and rel_l2(grads[0][n], grads[1][n]) < 1e-4, n


def _fp8_blocks(dev, mode, dgrad=False, r=24):
    """test_blocks_lora_tail's model with all eight targets: 2 + 2 blocks, frozen weights, adapters with zero_b=False and B x 10"""
    from vt355.hunyuan import HunyuanBlocks
    m = HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=2, mm_single_blocks_depth=2, fp8=mode, fp8_dgrad=dgrad, lora_rank=r,
                      lora_alpha=2.0, lora_target_modules=list(ALL)).to(dev).init_weights(4)
    m.lora.init_weights(5, zero_b=False)
    with torch.no_grad():
        for n, p in m.lora._plist.items():
            if ".lora_B" in n:
                p.mul_(10.0)
    return m, m.enable_lora_training()


# test_gradients_vs_mfma's rel-L2 caps of its LoRA case (tests/test_hunyuan_fp8_dgrad_gpu.py: _CAPS), cosine > 0.98 for every tensor
_DGRAD_CAPS = {"e5m2": 2 * 6.69e-2, "e4m3": 2 * 4.10e-2}


def test_fp8_matmul_mode_with_all_targets(dev):
    """fp8="matmul" (E4M3 weights everywhere, the qkv forward products on the fp8 matrix cores) at rank 24 with all eight targets: the image
    rows stay within test_double_then_single_stack_and_fp8_projection's bar of the bf16 model (8e-2), every adapter gradient is finite and
    non-zero"""
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    outs = {}
    for mode in (False, "matmul"):
        m, ts = _fp8_blocks(dev, mode)
        out = m(img, txt, vec, tv, (cos, sin))
        out.backward(dout)
        outs[mode] = out.detach()[:, :LI].float()
        assert torch.isfinite(ts.grad).all()
        for n in m.lora.shapes:
            assert m.lora._view(ts.grad, n).abs().max().item() > 0, n
    e = rel_l2(outs["matmul"], outs[False])
    print(f"[hunyuan lora ff matmul] image rows vs bf16 rel-L2 {e:.3e}")
    assert 0 < e < 8e-2


def test_fp8_mfma_against_weights_mode(dev):
    """fp8="mfma" at rank 24 with all targets against fp8="weights" (the same de-quantised weights, bf16 products), under
    test_blocks_lora_tail's bars: the adapters' contribution out(B) - out(B = 0) within 0.25 rel-L2 -- without the bf16 tails the adapted
    sites would contribute nothing (rel-L2 ~1) -- and every adapter gradient within 8e-2"""
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    res = {}
    for mode in ("weights", "mfma"):
        m, ts = _fp8_blocks(dev, mode)
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
        res[mode] = (o_b - o_0, {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}, o_b)
    contrib = rel_l2(res["mfma"][0], res["weights"][0])
    errs = sorted(((rel_l2(res["mfma"][1][n], res["weights"][1][n]), n) for n in res["weights"][1]), reverse=True)
    print(f"[hunyuan lora ff mfma] adapter contribution vs weights mode rel-L2 {contrib:.3e}; |contribution| {res['weights'][0].norm().item():.3e} of "
          f"|out| {res['weights'][2].norm().item():.3e}; worst adapter gradients vs weights {[(n, f'{a:.2e}') for a, n in errs[:4]]}")
    assert len(errs) == 2 * 22
    assert res["weights"][0].norm().item() > 0.05 * res["weights"][2].norm().item()
    assert contrib < 0.25 and errs[0][0] < 8e-2


def test_fp8_dgrad_against_mfma(dev):
    """test_fp8_mfma_and_dgrad_at_rank_64's criterion at rank 24 with all eight targets (the dGELU epilogue of vt_gemm_mxfp8_dx together with
    its bf16 tail): the forward is bit-equal with fp8_dgrad on and off (just-in-time and delayed-scale forward); with fp8_dgrad every adapter
    gradient and d(img), d(txt) stay within test_gradients_vs_mfma's LoRA bars of the fp8="mfma"-alone model, and the fp8 products did run"""
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs()]
    outs, grads = {}, {}
    for dg in (False, "e5m2", "e4m3"):
        m, ts = _fp8_blocks(dev, "mfma", dg)
        xi, xt = img.clone().requires_grad_(True), txt.clone().requires_grad_(True)
        o1 = m(xi, xt, vec, tv, (cos, sin))
        o1.backward(dout)
        with torch.no_grad():
            o2 = m(img, txt, vec, tv, (cos, sin))
        outs[dg] = (o1.detach().clone(), o2.clone())
        g = {n: m.lora._view(ts.grad, n).detach().clone() for n in m.lora.shapes}
        g["d(img)"], g["d(txt)"] = xi.grad.detach().clone(), xt.grad.detach().clone()
        grads[dg] = g
    ref, rows_of = grads[False], {}
    for fmt in ("e4m3", "e5m2"):                               # measure and print everything before the first assertion
        got = grads[fmt]
        rows = sorted(((rel_l2(got[n], ref[n]), cosine(got[n], ref[n]), n) for n in ref), reverse=True)
        rows_of[fmt] = rows
        wc = min(rows, key=lambda r_: r_[1])
        print(f"[hunyuan lora ff dgrad r24 {fmt}] {len(rows)} tensors; worst rel-L2 {rows[0][0]:.4e} ({rows[0][2]}); worst cosine {wc[1]:.5f} ({wc[2]})")
    for fmt in ("e4m3", "e5m2"):
        assert torch.equal(outs[fmt][0], outs[False][0]) and torch.equal(outs[fmt][1], outs[False][1])
        assert torch.isfinite(outs[fmt][0].float()).all()
        rows = rows_of[fmt]
        assert len(rows) == 2 * 22 + 2
        assert not any(torch.equal(grads[fmt][n], ref[n]) for n in ("d(img)", "d(txt)"))           # the fp8 dX products ran
        assert all(c > 0.98 for _, c, _ in rows), [x for x in rows if not x[1] > 0.98]
        assert rows[0][0] < _DGRAD_CAPS[fmt], rows[0]


# ---------------------------------------------------------------------------------------------------------------- 4: repack, partial backward
@pytest.mark.parametrize("r", [4, 24])
def test_repack_after_a_step_is_a_fresh_pack(dev, r):
    """after FusedAdamW.step() the extension columns / rows of every site are rewritten while the base columns stay: a freshly built model
    loaded from the stepped state dict (packed from scratch) gives the same forward bit for bit"""
    from vt355.optim import FusedAdamW
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs(21, 1, 40, 8)]
    m = _blocks(dev, r, ALL)
    ts = m.enable_lora_training()
    out = m(img, txt, vec, tv, (cos, sin))
    out.backward(dout)
    opt = FusedAdamW(ts.params, lr=1e-3, fullft_state=ts)
    before = ts.flat.clone()
    opt.step()
    assert torch.isfinite(ts.flat).all()
    for n in m.lora.shapes:                                        # every adapter moved
        assert (m.lora._view(ts.flat, n) - m.lora._view(before, n)).abs().max().item() > 0, n
    with torch.no_grad():
        out2 = m(img, txt, vec, tv, (cos, sin))
    assert not torch.equal(out2, out.detach())                    # the repacked adapters are used
    m2 = _blocks(dev, r, ALL, seed=99)
    m2.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()}, strict=True)
    m2.to(dev)
    with torch.no_grad():
        out3 = m2(img, txt, vec, tv, (cos, sin))
    assert torch.isfinite(out3.float()).all() and torch.equal(out3, out2)


@pytest.mark.parametrize("r", [4, 24])
def test_partial_backward_leaves_the_single_blocks_adapters_untouched(dev, r):
    """a loss on the double block's output only: the backward runs the double block's part of the tape, its adapters (attention group and
    fc1 / fc2) get gradients, the single block's -- q, k, v, mlp on linear1 and linear2's -- stay exactly zero"""
    from vt355.hunyuan import _HYRun
    img, txt, vec, tv, cos, sin, dout = [t.to(dev) for t in _inputs(22, 1, 40, 8)]
    m = _blocks(dev, r, ALL)
    ts = m.enable_lora_training()
    run = _HYRun(m, save=True)
    marks = []
    double = run.double_block

    def wrapped(*a, **k):
        iv, tv_ = double(*a, **k)
        marks.append((len(run.tape), iv, tv_))
        return iv, tv_
    run.double_block = wrapped
    run.forward(img, txt, vec, tv, (cos, sin))
    assert len(marks) == 1 and 0 < marks[0][0] < len(run.tape)
    n, iv, tv_ = marks[0]
    del run.tape[n:]
    iv.g, tv_.g = dout[:, :40].reshape(-1, D).contiguous(), dout[:, 40:].reshape(-1, D).contiguous()
    while run.tape:
        run.tape.pop()()
    run.lora_scatter()
    grads = {k: m.lora._view(ts.grad, k).detach().clone() for k in m.lora.shapes}
    touched = [k for k in grads if k.startswith("double_blocks.")]
    untouched = [k for k in grads if k.startswith("single_blocks.")]
    assert len(touched) == 12 and len(untouched) == 10
    for k in touched:
        assert torch.isfinite(grads[k]).all() and grads[k].abs().max().item() > 0, k
    for k in untouched:
        assert not bool(grads[k].any()), k


# ---------------------------------------------------------------------------------------------------------------- 5: the whole model
def test_whole_model_flow_training_step_with_all_targets(dev):
    """HYVideoDiffusionTransformer(lora_rank=24, all eight targets) at test_hunyuan_gpu's tiny size through HunyuanVideoFlow.training_step:
    the loss is finite, every adapter gradient is finite and non-zero"""
    import hunyuan_oracle as HO
    from vt355.hunyuan import HunyuanVideoFlow, HYVideoDiffusionTransformer
    m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=24, lora_alpha=2.0, lora_target_modules=list(ALL))
    m.load_state_dict(HO.init_model(HO.model_shapes(256, 2, 1, 1, 4, 4, (1, 2, 2), 64, 32), 3), strict=False)
    m.lora.init_weights(5, zero_b=False)
    m.to(dev)
    flow = HunyuanVideoFlow(model=m, learning_rate=1e-3).to(dev)
    flow.configure_optimizers()
    g = np.load(os.path.join(G, "hunyuan_model.npz"))
    T = lambda k: torch.from_numpy(g[k]).to(dev)
    batch = {"latents": T("x"), "prompt_embeds": T("text_states"), "prompt_attention_mask": T("text_mask"), "pooled_prompt_embeds": T("text_states_2")}
    torch.manual_seed(0)
    loss = flow.training_step(batch)
    loss.backward()
    ts = m.lora.train_state
    assert torch.isfinite(loss) and torch.isfinite(ts.grad).all()
    assert len(m.lora.shapes) == 22
    for n in m.lora.shapes:
        assert m.lora._view(ts.grad, n).abs().max().item() > 0, n


# ---------------------------------------------------------------------------------------------------------------- 6: sequence parallelism
def _sp_worker(rank, world, port, res):
    """test_hunyuan_sp_gpu._worker's LoRA run (2 + 2 blocks, rank 4) with all eight targets"""
    import torch.distributed as dist
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("VT355_LORA_WIDE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import vt355.hunyuan as hy
        _poison_engine(setattr)
        dev = torch.device("cuda:0")
        b, Li, Lt = 2, 96, 12
        m = hy.HunyuanBlocks(hidden_size=D, heads_num=H, mm_double_blocks_depth=2, mm_single_blocks_depth=2, lora_rank=4, lora_alpha=2.0,
                             lora_target_modules=list(ALL))
        m.init_weights(3)
        m.lora.init_weights(5, zero_b=False)
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
        res[rank] = errs
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_all_targets_under_ulysses_world2_match_unsharded(dev):
    """the two-rank run of test_hunyuan_sp_gpu with all eight targets: the new sites' adapter gradients are partial sums over a rank's rows
    (local image rows + the replicated text rows, whose incoming gradient rank 0 carries) as linear1's q / k / v adapters' are -- summed
    over the ranks they equal the unsharded run's, under that test's bars"""
    import torch.multiprocessing as mp
    from test_hunyuan_sp_gpu import _free_port
    mgr = mp.Manager(); res = mgr.dict()
    mp.spawn(_sp_worker, args=(2, _free_port(), res), nprocs=2, join=True)
    for r in (0, 1):
        print(f"[hunyuan sp-2 lora ff] rank {r}: " + ", ".join(f"{k} {v:.2e}" for k, v in res[r].items()))
        assert res[r].pop("zero_grads") == 0
        for k, v in res[r].items():
            assert v < (5e-2 if k == "worst_param" else 1e-2), (r, k, v)
