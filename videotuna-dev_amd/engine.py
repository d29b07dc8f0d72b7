"""Forward / backward schedule of the CogVideoX DiT on the HIP kernels (the hot loop of SURVEY.md 3.1:
``self.model(...)`` at videotuna/models/cogvideo_hf/cogvideo_pl.py:865-871 and the ``loss.backward()`` PL runs on it).

One autograd node covers the whole network: the forward launches the kernels and keeps the per-block
activations the backward needs (no per-block recomputation -- 288 GB of HBM holds ~27 GB/sample);
the backward walks the blocks in reverse, accumulates the LoRA gradients straight into the flat fp32 gradient
buffer (``+=`` semantics, so gradient accumulation over micro-batches is native) and returns no tensor grads.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import torch

from . import ops
from .lora import TARGETS
from .ops import BF16, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_GATED_RES

EXT = 64          # K-extension width without adapters and for LoRA ranks <= 16; wider ranks: LoraState.ext_qkv / ext_o
# q_hat is stored pre-multiplied by softmax_scale * log2(e) (head_dim 64) so the attention kernels exponentiate raw scores
Q_PRESCALE = 1.4426950408889634 / 8.0


def _lin(mod):
    """(weight, bias) of a Linear holder or of a LoRA-wrapped one."""
    base = getattr(mod, "base_layer", mod)
    return base.weight, base.bias


# ---------------------------------------------------------------------------------------------------
# operand packing
# ---------------------------------------------------------------------------------------------------
def _ext_widths(model):
    """(ext_qkv, ext_o): K-extension columns of the fused qkv / out operands (a property of the LoRA state's layout)"""
    st = model.lora
    return (st.ext_qkv, st.ext_o) if st is not None else (EXT, EXT)


def _ff_lora(model):
    """(ff.net.0.proj adapted, ff.net.2 adapted, K-extension columns of either): the feed-forward LoRA targets"""
    st = model.lora
    if st is None or not (getattr(st, "ff1", False) or getattr(st, "ff2", False)):
        return False, False, 0
    return st.ff1, st.ff2, st.ext_ff


def _dora(model):
    """the LoRA state when its adapters are weight-decomposed (LoraConfig.use_dora), else None"""
    st = model.lora
    return st if st is not None and getattr(st, "dora", False) else None


def _ext_rows(w: torch.Tensor, ext: int) -> torch.Tensor:
    """[N,K] -> [N,K+ext] with a zero K-extension."""
    out = torch.zeros(w.shape[0], w.shape[1] + ext, dtype=BF16, device=w.device)
    out[:, :w.shape[1]] = w
    return out


def _ext_t(w: torch.Tensor, ext: int) -> torch.Tensor:
    """[N,K] -> transposed [K+ext,N] with zero extension rows."""
    out = torch.zeros(w.shape[1] + ext, w.shape[0], dtype=BF16, device=w.device)
    out[:w.shape[1]] = w.t()
    return out


def pack(model) -> SimpleNamespace:
    ft = getattr(model, "fullft", None)
    if ft is None and any(p.requires_grad for n, p in model.named_parameters() if "lora" not in n):
        raise RuntimeError("base weights require grad but no training state exists: call vt355.fullft.enable_full_finetune(model) "
                           "for full fine-tuning, or freeze the base (requires_grad_(False)) and inject LoRA adapters")
    for n, p in model.named_parameters():
        if "lora" not in n and p.dtype != BF16:
            raise TypeError(f"parameter {n} is {p.dtype}; the MI355X engine computes in bf16 -- call .bfloat16()")
    eq, eo = _ext_widths(model)
    P = SimpleNamespace(layers=[], lora_version=-1, ft_version=-1 if ft is None else ft.version, ext=(eq, eo), ff=_ff_lora(model),
                        dora=_dora(model) is not None)
    ff1, ff2, ef = P.ff
    d = model.inner_dim
    with torch.no_grad():
        for i, blk in enumerate(model.transformer_blocks):
            a = blk.attn1
            wq, bq = _lin(a.to_q); wk, bk = _lin(a.to_k); wv, bv = _lin(a.to_v); wo, bo = _lin(a.to_out[0])
            L = SimpleNamespace()
            if ft is not None:
                # q|k|v weights / biases are adjacent in the flat buffer: the fused operand is a VIEW (no copy, no K-extension)
                pre = f"transformer_blocks.{i}.attn1."
                L.w_qkv = ft.span(ft.flat_bf16, pre + "to_q.weight", pre + "to_v.weight", (3 * d, d))
                L.b_qkv = ft.span(ft.flat_bf16, pre + "to_q.bias", pre + "to_v.bias", (3 * d,))
                L.w_qkv_t = L.w_qkv.t().contiguous()
                L.w_o, L.b_o, L.w_o_t = wo, bo, wo.t().contiguous()
            else:
                wqkv = torch.cat([wq, wk, wv], 0)
                L.w_qkv = _ext_rows(wqkv, eq); L.b_qkv = torch.cat([bq, bk, bv]).contiguous(); L.w_qkv_t = _ext_t(wqkv, eq)
                L.w_o = _ext_rows(wo, eo); L.b_o = bo; L.w_o_t = _ext_t(wo, eo)
                if P.dora:
                    # DoRA rescales the operands from the pristine weights at every adapter version (_dora_refresh): the fused q | k | v
                    # weight stays as one more copy (3 d^2 bf16 per layer; the other Linears' pristine weights are their parameters) beside
                    # the factors c = m / ||W + s B A|| of each projection, 1 where a Linear is not adapted
                    L.w_qkv0 = wqkv
                    L.c_qkv, L.c_o = (torch.ones(n, dtype=torch.float32, device=wo.device) for n in (3 * d, d))
            w1, b1 = _lin(blk.ff.net[0].proj); w2, b2 = _lin(blk.ff.net[2])
            L.w1, L.b1, L.w1_t = w1, b1, w1.t().contiguous()
            L.w2, L.b2, L.w2_t = w2, b2, w2.t().contiguous()
            if ff1:         # ff.net.0.proj adapted: both operands of W1 carry the K-extension, as the attention projections' do
                L.w1, L.w1_t = _ext_rows(w1, ef), _ext_t(w1, ef)
            if ff2:
                # ff.net.2 adapted.  Forward: [W2 | s B2].  Backward: du = gelu'(u) (x) ([tg | dt2] [W2^T | A2^T]^T), the adapter's input-gradient
                # correction as a K-extension of the product that carries the dGELU epilogue; dt2 = tg (s B2) from w2_bt [ext, d].
                L.w2 = _ext_rows(w2, ef)
                L.w2_t = _ext_rows(L.w2_t, ef)
                L.w2_bt = torch.zeros(ef, w2.shape[0], dtype=BF16, device=w2.device)
            if P.dora:
                L.c_1 = torch.ones(w1.shape[0], dtype=torch.float32, device=w1.device) if ff1 else None
                L.c_2 = torch.ones(w2.shape[0], dtype=torch.float32, device=w2.device) if ff2 else None
            L.n1g, L.n1b = blk.norm1.norm.weight, blk.norm1.norm.bias
            L.n2g, L.n2b = blk.norm2.norm.weight, blk.norm2.norm.bias
            L.gq, L.bq, L.gk, L.bk = a.norm_q.weight, a.norm_q.bias, a.norm_k.weight, a.norm_k.bias
            P.layers.append(L)
        if ft is not None:
            nl = model.config.num_layers
            nmod = (12 * nl + 2) * d
            P.w_ada = ft.span(ft.flat_bf16, "transformer_blocks.0.norm1.linear.weight", "norm_out.linear.weight",
                              (nmod, model.config.time_embed_dim))
            P.b_ada = ft.span(ft.flat_bf16, "transformer_blocks.0.norm1.linear.bias", "norm_out.linear.bias", (nmod,))
        else:
            ada_w = [m.linear.weight for blk in model.transformer_blocks for m in (blk.norm1, blk.norm2)]
            ada_b = [m.linear.bias for blk in model.transformer_blocks for m in (blk.norm1, blk.norm2)]
            P.w_ada = torch.cat(ada_w + [model.norm_out.linear.weight], 0).contiguous()
            P.b_ada = torch.cat(ada_b + [model.norm_out.linear.bias], 0).contiguous()
        pw = model.patch_embed.proj.weight
        P.patch_w = pw.reshape(pw.shape[0], -1).contiguous()            # [d, C*p*p]  (c p q)
        P.patch_b = model.patch_embed.proj.bias
        P.text_w, P.text_b = _lin(model.patch_embed.text_proj)
        P.t1_w, P.t1_b = _lin(model.time_embedding.linear_1)
        P.t2_w, P.t2_b = _lin(model.time_embedding.linear_2)
        P.proj_w, P.proj_b = _lin(model.proj_out)
        P.proj_w_t = P.proj_w.t().contiguous()                          # [d, C*p*p]
    return P


def packed(model) -> SimpleNamespace:
    ft = getattr(model, "fullft", None)
    if (model._packed is None or (ft is not None and model._packed.ft_version != ft.version)
            or model._packed.ext != _ext_widths(model) or model._packed.ff != _ff_lora(model)
            or model._packed.dora != (_dora(model) is not None)):
        model._packed = pack(model)          # full fine-tune: the transposed operand copies follow the updated weights
    P = model._packed
    st = model.lora
    if st is not None and P.lora_version != st.version:
        d, r, rp, eq, eo = model.inner_dim, st.r, st.rp, st.ext_qkv, st.ext_o
        ff1, ff2, ef = P.ff
        # feed-forward targets: one adapter per Linear, packed by the kernels that pack to_out.0's
        if st.wide:
            pack_b = lambda b, w, ld, n: ops.lora_pack_b_wide(b, w, ld, 1, n, r, rp, ef, st.scaling)
            pack_bt = lambda b, w, ld, n: ops.lora_pack_bt_wide(b, w, ld, 1, n, r, rp, ef, st.scaling)
        else:
            pack_b = lambda b, w, ld, n: ops.lora_pack_b(b, w, ld, 1, n, r, st.scaling)
            pack_bt = lambda b, w, ld, n: ops.lora_pack_bt(b, w, ld, 1, n, r, st.scaling)
        for i, L in enumerate(P.layers):
            if ff1:
                dff, b1 = L.w1.shape[0], st.view(st.flat, i, "B", 4)
                pack_b(b1, L.w1[:, d:], d + ef, dff)
                pack_bt(b1, L.w1_t[d:], dff, dff)
            if ff2:
                dff, b2 = L.w2_t.shape[0], st.view(st.flat, i, "B", 5)
                pack_b(b2, L.w2[:, dff:], dff + ef, d)
                pack_bt(b2, L.w2_bt, d, d)
                L.w2_t[:, d:d + r].copy_(ops.transpose(st.view(st.flat_bf16, i, "A", 5)))       # A2^T: rank column i <- row i of A2
            if st.wide:
                ops.lora_pack_b_wide(st.b_qkv(st.flat, i), L.w_qkv[:, d:], d + eq, 3, d, r, rp, eq, st.scaling)
                ops.lora_pack_bt_wide(st.b_qkv(st.flat, i), L.w_qkv_t[d:], 3 * d, 3, d, r, rp, eq, st.scaling)
                ops.lora_pack_b_wide(st.b_out(st.flat, i), L.w_o[:, d:], d + eo, 1, d, r, rp, eo, st.scaling)
                ops.lora_pack_bt_wide(st.b_out(st.flat, i), L.w_o_t[d:], d, 1, d, r, rp, eo, st.scaling)
                continue
            ops.lora_pack_b(st.b_qkv(st.flat, i), L.w_qkv[:, d:], d + eq, 3, d, r, st.scaling)
            ops.lora_pack_bt(st.b_qkv(st.flat, i), L.w_qkv_t[d:], 3 * d, 3, d, r, st.scaling)
            ops.lora_pack_b(st.b_out(st.flat, i), L.w_o[:, d:], d + eo, 1, d, r, st.scaling)
            ops.lora_pack_bt(st.b_out(st.flat, i), L.w_o_t[d:], d, 1, d, r, st.scaling)
        if P.dora:
            for i, L in enumerate(P.layers):
                _dora_refresh(model, st, i, L, P.ff)
        P.lora_version = st.version
    return P


# DoRA (DESIGN 3 "DoRA"): y = b + c (x) (W x + s B A x), c_j = m_j / ||W_j + s (B A)_j|| with the norm detached.  The extended products
# already compute W x + s B A x in one GEMM, so c is folded into the operands: forward [c W | c s B]; of the transposed operands that
# multiply the output gradient g, the base part indexed by the output feature and the s B^T extension rows (w2_bt for ff.net.2), which
# makes dx and dT = g' (s B), g' = c (x) g, and with them dA, the plain LoRA backward on g'.  Only dB = diag(c) s g^T T (_lora_db) and the
# magnitude gradient (_dora_dm) need kernels of their own.  The fold runs here, once per adapter version (an optimizer step or a load).
def _dora_fold(st, w0, a, b, n, mag, c, w_fwd, wt_base, wt_ext, not_adapted=()):
    """c = mag / ||w0 + s b a|| (1 on the rows of not_adapted), then the four operand parts of one projection: the base columns of w_fwd and
    the base part wt_base of the transposed operand from the pristine w0 [N, K], their extension parts (just written by the pack kernels
    from the masters) in place"""
    K = w0.shape[1]
    ops.dora_norm(w0, a, b, n, st.r, st.scaling, c, mag=mag)
    for rows in not_adapted:
        c[rows].fill_(1.0)
    ops.dora_scale(w0, w_fwd[:, :K], c)
    ops.dora_scale(w_fwd[:, K:], w_fwd[:, K:], c)
    ops.dora_transpose_scale(w0, wt_base, c)
    ops.dora_scale(wt_ext, wt_ext, c, by_col=True)


def _dora_refresh(model, st, i, L, ff):
    d, bf = model.inner_dim, st.flat_bf16
    ff1, ff2, _ = ff
    blk = model.transformer_blocks[i]
    qkv = [t in st.targets for t in ("to_q", "to_k", "to_v")]
    if any(qkv):
        _dora_fold(st, L.w_qkv0, st.a_qkv(bf, i), st.b_qkv(bf, i), 3, st.mag_qkv(st.flat, i), L.c_qkv, L.w_qkv, L.w_qkv_t[:d], L.w_qkv_t[d:],
                   [slice(j * d, (j + 1) * d) for j in range(3) if not qkv[j]])
    if "to_out.0" in st.targets:
        _dora_fold(st, _lin(blk.attn1.to_out[0])[0], st.a_out(bf, i), st.b_out(bf, i), 1, st.view(st.flat, i, "M", 3), L.c_o, L.w_o,
                   L.w_o_t[:d], L.w_o_t[d:])
    if ff1:
        _dora_fold(st, _lin(blk.ff.net[0].proj)[0], st.view(bf, i, "A", 4), st.view(bf, i, "B", 4), 1, st.view(st.flat, i, "M", 4), L.c_1,
                   L.w1, L.w1_t[:d], L.w1_t[d:])
    if ff2:         # the transposed operand is [W2^T | A2^T]: its extension columns multiply dT2 and stay; dT2 = tg (c s B2) comes from w2_bt
        _dora_fold(st, _lin(blk.ff.net[2])[0], st.view(bf, i, "A", 5), st.view(bf, i, "B", 5), 1, st.view(st.flat, i, "M", 5), L.c_2,
                   L.w2, L.w2_t[:, :d], L.w2_bt)


def _lora_db(st, tn, big, small, gB, P, c=None):
    """dB += s big^T small (small: the saved T).  DoRA (c: the projection's factors): dB += diag(c) s big^T small -- the tn kernels have no
    row factor, so the product goes to a zeroed scratch and vt_dora_db_add adds it scaled.  gB [n P, r]: adapter j of a fused projection
    (qkv: n = 3) owns columns [j P, (j+1) P) of big, the extension columns from j rp of small and rows [j P, (j+1) P) of gB."""
    out = gB if c is None else st.dora_scratch(gB.numel()).view(gB.shape)
    for j in range(gB.shape[0] // P):
        tn(big[:, j * P:], small[:, j * st.rp:], st.r, out[j * P:], st.r, 1, st.scaling, P)
    if c is not None:
        ops.dora_db_add(gB, out, c)


def _dora_dm(st, i, j, g, y, bias, n=1):
    """dm += (sum_m g y - b sum_m g) / m for Linear j of layer i (n = 3: the fused q | k | v projection, from one pass over g and y; only
    the adapted ones own a magnitude); g: the gradient of the Linear's output y [M, N], y with the bias"""
    N = g.shape[1]
    sums = st.dora_scratch(2 * N)
    ops.group_colsum(g, sums[:N], y=y, out2=sums[N:])
    d = N // n
    for k in range(n):
        if TARGETS[j + k] in st.targets:
            cols = slice(k * d, (k + 1) * d)
            ops.dora_dm(sums[:N][cols], sums[N:][cols], None if bias is None else bias[cols], st.view(st.flat, i, "M", j + k),
                        st.view(st.grad, i, "M", j + k))


# The rank-side products of the two adapted projections of a block -- "qkv": the three adapters of the fused q | k | v projection,
# "out": the one of to_out.0 -- each issued from one place: _lora_down, _lora_da, _lora_dx.  They choose the layout (ranks <= 16: the
# narrow kernels of csrc/lora.hip, ranks 17..128 (st.wide): the MFMA kernels of csrc/lora_wide.hip, every adapter of a projection in one
# pass over the activation) and whether the dropped kernels run.
#
# lora_dropout: ``drop`` is None or (p, seed) of the forward in flight; the adapter sites of layer i are 4 i + {0, 1, 2, 3} for
# to_q, to_k, to_v, to_out.0 and every site has its own keep mask.  With drop the dropped kernels run (same passes over the activation,
# the mask recomputed in the kernel); without it the calls are exactly the ones made before lora_dropout existed.
def lora_dropout_seed(model):
    """(p, seed) for one training forward of a model whose adapters have lora_dropout > 0, else None.  model.lora_dropout_seed pins the
    seed; None draws a fresh one per forward from torch's CPU generator (every rank of a data-parallel job draws its own)."""
    st = model.lora
    if st is None or not getattr(st, "p", 0.0) or not model.training:
        return None
    seed = getattr(model, "lora_dropout_seed", None)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    model.last_lora_dropout_seed = int(seed)
    return float(st.p), int(seed)


def _lora_proj(st, i, proj, buf):
    """(adapters, their stacked A rows [n r, d] in buf, K-extension width, site of the first adapter) of projection ``proj`` of layer i"""
    if proj == "qkv":
        return 3, st.a_qkv(buf, i), st.ext_qkv, 4 * i
    if proj == "ff1":          # ff.net.0.proj / ff.net.2: their sites follow every attention site, so those masks do not move
        return 1, st.view(buf, i, "A", 4), st.ext_ff, 4 * st.L + 2 * i
    if proj == "ff2":
        return 1, st.view(buf, i, "A", 5), st.ext_ff, 4 * st.L + 2 * i + 1
    return 1, st.a_out(buf, i), st.ext_o, 4 * i + 3


def _narrow_calls(n, r):
    """(first adapter, adapters) of each call of a narrow rank-side kernel.  These take at most 16 rank columns, so the adapters of a
    fused projection share one call up to 3 r <= 16 (the shipped recipes, r = 4) and get a call each on their r columns above that."""
    return [(0, n)] if n * r <= 16 else [(j, 1) for j in range(n)]


def _lora_down(st, i, proj, x, d, drop=None):
    """T = x A^T (drop: of x under each adapter's mask) into the K-extension columns x[:, d:], zeros in the columns no adapter owns"""
    n, a, ext, site = _lora_proj(st, i, proj, st.flat_bf16)
    r, rp = st.r, st.rp
    if st.wide:
        if drop is None:
            ops.lora_down_wide(x, a, n, r, rp, ext, x[:, d:], d)
        elif ops.lora_down_wide_drop_fits(n, rp):
            ops.lora_down_wide_drop(x, a, n, r, rp, ext, x[:, d:], d, *drop, site)
        else:
            # one masked copy of the X block per adapter does not fit the LDS (3 adapters, rp > 80): a call per adapter on its rp
            # columns, the last one zeroes the rest of the extension
            for j in range(n):
                ops.lora_down_wide_drop(x, a[j * r:(j + 1) * r], 1, r, rp, rp if j < n - 1 else ext - j * rp, x[:, d + j * rp:], d,
                                        *drop, site + j)
        return
    for j, nj in _narrow_calls(n, r):
        # a call writes 16 columns from j r (zeros past its rows; the next call overwrites them), the last one zeroes the rest
        zc = EXT - 16 - j * r if j + nj == n else 0
        if drop is None:
            ops.lora_down(x, a[j * r:(j + nj) * r], nj * r, x[:, d + j * r:], d, zero_cols=zc)
        else:
            ops.lora_down_drop(x, a[j * r:(j + nj) * r], nj * r, nj, x[:, d + j * r:], d, *drop, site + j, zero_cols=zc)


def _lora_da(st, i, proj, x, dxe, d, drop=None, dt0=None):
    """dA += dT^T x (drop: x under each adapter's mask); x: the projection's input, dT: the extension columns of dxe [M, d + ext]
    (dt0: dT where it lives elsewhere -- ff.net.2, whose dT sits beside the output gradient, not beside dx)"""
    n, ga, _, site = _lora_proj(st, i, proj, st.grad)
    r = st.r
    for j, nj in ([(j, 1) for j in range(n)] if st.wide else _narrow_calls(n, r)):          # lora_tn_wide: one adapter per call
        dt, g = (dxe[:, d + j * st.rp:] if dt0 is None else dt0[:, j * st.rp:]), ga[j * r:(j + nj) * r]
        if st.wide and drop is None:
            ops.lora_tn_wide(x, dt, r, g, 1, d, 1.0, d)
        elif st.wide:
            ops.lora_tn_wide_drop(x, dt, r, g, 1, d, 1.0, d, *drop, site + j)
        elif drop is None:
            ops.skinny_tn(x, dt, nj * r, g, 1, d, 1.0, d)
        else:
            ops.skinny_tn_drop(x, dt, nj * r, nj, g, 1, d, 1.0, d, *drop, site + j)


def _lora_dx(st, i, proj, dxe, d, drop=None):
    """dxe[:, :d] += dT A (drop: each adapter's term under its mask), dT = the extension columns of dxe"""
    n, a, _, site = _lora_proj(st, i, proj, st.flat_bf16)
    r = st.r
    if st.wide:
        if drop is None:
            ops.lora_up_add_wide(dxe, dxe[:, d:], a, n, r, st.rp, d)
        else:
            ops.lora_up_add_wide_drop(dxe, dxe[:, d:], a, n, r, st.rp, d, *drop, site)
        return
    for j, nj in _narrow_calls(n, r):
        if drop is None:
            ops.lora_up_add(dxe, dxe[:, d + j * r:], a[j * r:(j + nj) * r], nj * r, d)
        else:
            ops.lora_up_add_drop(dxe, dxe[:, d + j * r:], a[j * r:(j + nj) * r], nj * r, nj, d, *drop, site + j)


def _lora_dx_dgelu(st, i, du, dt, u, K, drop):
    """du += gelu'(u) (x) keep (x) (dT A2) / (1 - p): ff.net.2's dX correction under lora_dropout.  The mask sits between dT A2 and the GELU, so
    the term cannot ride in the K-extension of the W2^T product as it does without dropout; du already carries gelu'(u) (x) (tg W2)."""
    _, a, _, site = _lora_proj(st, i, "ff2", st.flat_bf16)
    if st.wide:
        ops.lora_up_add_wide_dgelu_drop(du, dt, a, 1, st.r, st.rp, u, K, *drop, site)
    else:
        ops.lora_up_add_dgelu_drop(du, dt, a, st.r, 1, u, K, *drop, site)


# Aliases that only tests/test_side_kernels_gpu.py calls; they go when its call sites move to the helpers above.
def _lora_down_qkv(x1, st, i, d, drop=None):
    """the qkv down-projection by its earlier name"""
    _lora_down(st, i, "qkv", x1, d, drop)


def _lora_qkv_input_grads(x1, dx1, st, i, d, need_dx=True, drop=None):
    """dA_qkv += dT^T x1 and (need_dx) dx1 += dT A_qkv by their earlier name (see _lora_down_qkv)"""
    _lora_da(st, i, "qkv", x1, dx1, d, drop)
    if need_dx:
        _lora_dx(st, i, "qkv", dx1, d, drop)


def _mod(mod: torch.Tensor, idx: int, d: int):
    """six fp32 views into the modulation table for LayerNormZero number idx: chunk order
    shift, scale, gate, enc_shift, enc_scale, enc_gate (video first, then text)."""
    o = idx * 6 * d
    v = lambda k: mod[:, o + k * d:]
    return SimpleNamespace(shift_vid=v(0), scale_vid=v(1), gate_vid=v(2), shift_txt=v(3), scale_txt=v(4), gate_txt=v(5),
                           bs=mod.stride(0))


def saved_bytes_per_block(model, M: int) -> int:
    """activation bytes one block keeps for its backward pass (bf16 rows of width d unless noted)"""
    d = model.inner_dim
    ext2 = sum(_ext_widths(model)) if model.lora is not None else 0         # x1 carries ext_qkv extra columns, o ext_o
    cols = 2 * d + ext2 + 3 * d + 2 * d + d + model.config.ff_mult * d + d         # x1, o | qkv | qkh | h1 | u | h_in
    if getattr(model, "fullft", None) is not None:
        cols += d + model.config.ff_mult * d + 2 * d                                  # x2 | g | ao, fo
    ff1, ff2, ef = _ff_lora(model)             # an adapted feed-forward Linear keeps its input (dA) with the K-extension (dB)
    cols += (d + ef if ff1 else 0) + (model.config.ff_mult * d + ef if ff2 else 0)
    dora = _dora(model)
    if dora is not None:                       # dm of to_out.0 / ff.net.2 reads the branch output before gating: ao / fo
        cols += (d if "to_out.0" in dora.targets else 0) + (d if ff2 else 0)
    return M * cols * 2


def _use_recompute(model, dims) -> bool:
    """Per-block activation recompute (the reference's enable_gradient_checkpointing(), cogvideo_pl.py:141).
    ``model.recompute``: "never" | "always" | "auto" (default once enable_gradient_checkpointing() was called: recompute only
    when the kept activations would not fit comfortably in the free HBM -- on a 288 GB MI355X the benchmark configuration
    keeps them: -25 % executed FLOPs).  VT355_RECOMPUTE overrides."""
    import os
    mode = os.environ.get("VT355_RECOMPUTE") or getattr(model, "recompute", "never")
    if mode == "always":
        return True
    if mode != "auto":
        return False
    need = saved_bytes_per_block(model, dims[-1]) * model.config.num_layers
    free, _ = torch.cuda.mem_get_info()
    return need > 0.6 * free


def block_forward(model, i: int, h, mod, dims, rope, save: bool, scratch, drop=None):
    """One CogVideoXBlock forward (diffusers CogVideoXBlock via cogvideo_pl.py:865-871): returns (h_out, a) where a holds
    what the block's backward needs (only ``h_in`` unless ``save``).  Called again from the backward pass when the block's
    activations are recomputed instead of kept, with the ``drop`` = (p, seed) of the first pass: the same lora_dropout masks."""
    c = model.config
    P = packed(model)
    st = model.lora
    ft = getattr(model, "fullft", None)
    d, H = model.inner_dim, c.num_attention_heads
    B, Fr, C, Hh, Ww, S, St, Sv, M = dims
    dev = h.device
    eq, eo = _ext_widths(model)
    KEq, KEo = (d + eq, d + eo) if st is not None else (d, d)        # GEMM reduction lengths on the LoRA-extended operands
    E = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
    xg, gbuf = scratch.xg, scratch.gbuf
    Lw = P.layers[i]
    m1, m2 = _mod(mod, 2 * i, d), _mod(mod, 2 * i + 1, d)
    a = SimpleNamespace(h_in=h)
    # --- attention branch ---
    x1 = E(M, d + eq)
    a.mean1, a.rstd1 = E(M, dt=torch.float32), E(M, dt=torch.float32)
    ops.ln_modulate_fwd(h, x1, Lw.n1g, Lw.n1b, (m1.shift_txt, m1.scale_txt, m1.shift_vid, m1.scale_vid, m1.bs),
                        a.mean1, a.rstd1, d, S, St, c.norm_eps)
    if st is not None:
        _lora_down(st, i, "qkv", x1, d, drop)
    qkv = E(M, 3 * d)
    ops.gemm(x1, Lw.w_qkv, qkv, Lw.b_qkv, K=KEq)
    qkh = E(M, 2 * d)
    a.qmean, a.qrstd = E(M, 2 * H, dt=torch.float32), E(M, 2 * H, dt=torch.float32)
    ops.qk_layernorm_fwd(qkv, qkh, Lw.gq, Lw.bq, Lw.gk, Lw.bk, a.qmean, a.qrstd, H, 1e-6, q_scale=Q_PRESCALE, rope=rope)
    o = E(M, d + eo)
    lse = E(B, H, S, dt=torch.float32)
    qk3, qkv3, o3 = qkh.view(B, S, 2 * d), qkv.view(B, S, 3 * d), o.view(B, S, d + eo)
    ops.attn_fwd(qk3[:, :, :d], qk3[:, :, d:], qkv3[:, :, 2 * d:], o3[:, :, :d], lse, B, H, S, q_prescaled=True)
    if st is not None:
        _lora_down(st, i, "out", o, d, drop)
    h1 = E(M, d)
    dora = _dora(model)                                            # DoRA: dm of to_out.0 / ff.net.2 needs their outputs y = ao / fo too
    ao = E(M, d) if (save and (ft is not None or (dora is not None and "to_out.0" in dora.targets))) else None    # branch output before gating (gate gradient)
    ops.gemm(o, Lw.w_o, h1, Lw.b_o, epilogue=EPI_GATED_RES, residual=h, gate_txt=m1.gate_txt, gate_vid=m1.gate_vid,
             gate_bstride=m1.bs, S=S, St=St, K=KEo, pre_act_out=ao)
    # --- feed-forward branch ---
    a.mean2, a.rstd2 = E(M, dt=torch.float32), E(M, dt=torch.float32)
    keep_ff = save and ft is not None                              # dW1 / dW2 need the FF inputs
    ff1, ff2, ef = _ff_lora(model)                                 # LoRA on ff.net.0.proj / ff.net.2: x2 / gact carry a K-extension
    dff = c.ff_mult * d
    x2 = E(M, d + ef if ff1 else d) if (keep_ff or (save and ff1)) else xg          # an adapted Linear's input is kept for dA, dB
    gact = E(M, dff + ef if ff2 else dff) if (keep_ff or (save and ff2)) else gbuf
    ops.ln_modulate_fwd(h1, x2, Lw.n2g, Lw.n2b, (m2.shift_txt, m2.scale_txt, m2.shift_vid, m2.scale_vid, m2.bs),
                        a.mean2, a.rstd2, d, S, St, c.norm_eps)
    if ff1:
        _lora_down(st, i, "ff1", x2, d, drop)
    u = E(M, dff) if save else gbuf.new_empty(M, dff)
    ops.gemm(x2, Lw.w1, gact, Lw.b1, epilogue=EPI_BIAS_GELU, pre_act_out=u, K=d + ef if ff1 else None)
    if ff2:
        _lora_down(st, i, "ff2", gact, dff, drop)
    h2 = E(M, d)
    fo = E(M, d) if (keep_ff or (save and dora is not None and ff2)) else None
    k2 = dff + ef if ff2 else dff
    ops.gemm(gact, Lw.w2, h2, Lw.b2, epilogue=EPI_GATED_RES, residual=h1, gate_txt=m2.gate_txt, gate_vid=m2.gate_vid,
             gate_bstride=m2.bs, S=S, St=St, pre_act_out=fo, K=k2, tile=ops.gemm_block_tile(M, d, k2))
    if save:
        a.x1, a.qkv, a.qkh, a.o, a.lse, a.h1, a.u = x1, qkv, qkh, o, lse, h1, u
        a.x2, a.g, a.ao, a.fo = (x2, gact, ao, fo) if ft is not None else (x2 if ff1 else None, gact if ff2 else None, ao, fo)
    return h2, a


# ---------------------------------------------------------------------------------------------------
def run_forward(model, x, text, t, save: bool, rope=None):
    c = model.config
    P = packed(model)
    st = model.lora
    d, H, L = model.inner_dim, c.num_attention_heads, c.num_layers
    B, Fr, C, Hh, Ww = x.shape
    p = c.patch_size
    Sv, St = Fr * (Hh // p) * (Ww // p), text.shape[1]
    S = St + Sv
    M = B * S
    dev = x.device
    ft = getattr(model, "fullft", None)
    E = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)

    # ---- time embedding + every adaLN modulation of the network in one GEMM ----
    te = c.time_embed_dim
    tsin = E(B, d); ops.timestep_embedding(t, tsin, c.flip_sin_to_cos, float(c.freq_shift))
    e1_pre = E(B, te); ops.gemm(tsin, P.t1_w, e1_pre, P.t1_b)
    e1 = E(B, te); ops.silu(e1_pre, e1)
    emb_pre = E(B, te); ops.gemm(e1, P.t2_w, emb_pre, P.t2_b)
    emb = E(B, te); ops.silu(emb_pre, emb)                # every consumer applies SiLU(emb) first
    mod = E(B, P.w_ada.shape[0], dt=torch.float32); ops.gemm(emb, P.w_ada, mod, P.b_ada)

    # ---- patch / text embedding into the joint [text, video] sequence ----
    h = E(M, d)
    patches = E(B * Sv, C * p * p); ops.patchify(x, patches, p)
    pos = model.pos_table(Fr, Hh, Ww, dev)          # None: RoPE model without a learned table
    pos_txt = model.patch_embed.pos_embedding[0, :St] if c.use_learned_positional_embeddings else None
    for b in range(B):
        if pos is not None:
            ops.gemm(patches[b * Sv:(b + 1) * Sv], P.patch_w, h[b * S + St:(b + 1) * S], P.patch_b,
                     epilogue=EPI_GATED_RES, residual=pos)
        else:
            ops.gemm(patches[b * Sv:(b + 1) * Sv], P.patch_w, h[b * S + St:(b + 1) * S], P.patch_b)
        if pos_txt is not None:
            ops.gemm(text[b], P.text_w, h[b * S:b * S + St], P.text_b, epilogue=EPI_GATED_RES, residual=pos_txt)
        else:
            ops.gemm(text[b], P.text_w, h[b * S:b * S + St], P.text_b)
    if rope is not None:
        rope = (rope[0], rope[1], S, St)

    dims = (B, Fr, C, Hh, Ww, S, St, Sv, M)
    ff1, ff2, ef = _ff_lora(model)
    scratch = SimpleNamespace(xg=E(M, d + ef if ff1 else d),            # transient: norm2 output, GELU output (each with the K-extension
                              gbuf=E(M, c.ff_mult * d + (ef if ff2 else 0)))           # of its Linear when that one is adapted)
    recompute = save and _use_recompute(model, dims)
    drop = lora_dropout_seed(model)         # None unless lora_dropout > 0 and model.training
    saved: List[SimpleNamespace] = []
    for i in range(L):
        h2, a = block_forward(model, i, h, mod, dims, rope, save and not recompute, scratch, drop)
        if save:
            saved.append(a)         # recompute: only the block input (a.h_in), the rest is rebuilt in the backward pass
        h = h2

    # ---- final: norm_final (video rows) -> AdaLayerNorm(shift, scale) -> proj_out -> unpatchify ----
    mo = 2 * L * 6 * d
    f_shift, f_scale = mod[:, mo:], mod[:, mo + d:]
    y1 = E(B * Sv, d); y2 = E(B * Sv, d)
    fm1, fr1 = E(B * Sv, dt=torch.float32), E(B * Sv, dt=torch.float32)
    fm2, fr2 = E(B * Sv, dt=torch.float32), E(B * Sv, dt=torch.float32)
    for b in range(B):
        rows = slice(b * Sv, (b + 1) * Sv)
        ops.ln_modulate_fwd(h[b * S + St:(b + 1) * S], y1[rows], model.norm_final.weight, model.norm_final.bias, None,
                            fm1[rows], fr1[rows], d, Sv, 0, c.norm_eps)
    ops.ln_modulate_fwd(y1, y2, model.norm_out.norm.weight, model.norm_out.norm.bias,
                        (f_shift, f_scale, f_shift, f_scale, mod.stride(0)), fm2, fr2, d, Sv, 0, c.norm_eps)
    tok = E(B * Sv, P.proj_w.shape[0])
    ops.gemm(y2, P.proj_w, tok, P.proj_b)
    out = E(B, Fr, c.out_channels, Hh, Ww)
    ops.unpatchify(tok, out, p)
    ctx = None
    if save:
        ctx = SimpleNamespace(blocks=saved, mod=mod, h_last=h, y1=y1, fm1=fm1, fr1=fr1, fm2=fm2, fr2=fr2,
                              dims=dims, f_scale=f_scale, rope=rope, recompute=recompute, scratch=scratch if recompute else None,
                              lora_drop=drop)
        if ft is not None:
            ctx.y2, ctx.tsin, ctx.e1_pre, ctx.e1, ctx.emb_pre, ctx.se, ctx.patches, ctx.text = y2, tsin, e1_pre, e1, emb_pre, emb, patches, text
    return out, ctx


def run_backward(model, ctx, dout: torch.Tensor):
    c = model.config
    P = packed(model)
    st = model.lora
    d, H, L = model.inner_dim, c.num_attention_heads, c.num_layers
    B, Fr, C, Hh, Ww, S, St, Sv, M = ctx.dims
    p = c.patch_size
    dev = dout.device
    eq, eo = st.ext_qkv, st.ext_o
    tn = ops.lora_tn_wide if st.wide else ops.skinny_tn       # dB products (they read the saved T: no mask): MFMA kernel above rank 16
    E = lambda *s, dt=BF16: torch.empty(*s, dtype=dt, device=dev)
    mod = ctx.mod
    drop = ctx.lora_drop          # (p, seed) of this forward's lora_dropout masks, or None
    dora = _dora(model) is not None          # DoRA: dB takes the row factor c (_lora_db), every adapted Linear a magnitude gradient (_dora_dm)

    # ---- final layers ----
    dtok = E(B * Sv, c.out_channels * p * p); ops.patchify(dout, dtok, p)
    dy2 = E(B * Sv, d); ops.gemm(dtok, P.proj_w_t, dy2, None)
    dy1 = E(B * Sv, d)
    ops.ln_modulate_bwd(dy2, ctx.y1, ctx.fm2, ctx.fr2, model.norm_out.norm.weight, (ctx.f_scale, ctx.f_scale, mod.stride(0)),
                        None, dy1, d, Sv, 0)
    dh = torch.zeros(M, d, dtype=BF16, device=dev)          # text rows of the last block get no gradient (2B)
    for b in range(B):
        rows = slice(b * Sv, (b + 1) * Sv)
        ops.ln_modulate_bwd(dy1[rows], ctx.h_last[b * S + St:(b + 1) * S], ctx.fm1[rows], ctx.fr1[rows],
                            model.norm_final.weight, None, None, dh[b * S + St:(b + 1) * S], d, Sv, 0)

    # ---- transient buffers shared by all blocks ----
    ff1, ff2, ef = _ff_lora(model)
    dff = c.ff_mult * d
    tg = E(M, d)
    tgf = E(M, d + ef) if ff2 else tg            # ff.net.2 adapted: the feed-forward branch's output gradient as [tg | dT2]
    du = E(M, dff)
    dx2 = E(M, d + ef) if ff1 else E(M, d)       # ff.net.0.proj adapted: [dx2 | dT1]
    dh1 = E(M, d)
    dO = E(M, d + eo)
    dq = E(B, S, d, dt=torch.float32)
    dkh = E(M, d)
    dqkv = E(M, 3 * d)
    dx1 = E(M, d + eq)
    delta = E(B * H * S, dt=torch.float32)
    chain_ws = ops.attn_bwd_chain_workspace(B, H, S, dev)
    dh_in = E(M, d)
    for i in reversed(range(L)):
        Lw, a = P.layers[i], ctx.blocks[i]
        if ctx.recompute:           # rebuild this block's activations from its input
            _, a = block_forward(model, i, a.h_in, mod, ctx.dims, ctx.rope, True, ctx.scratch, drop)
        m1, m2 = _mod(mod, 2 * i, d), _mod(mod, 2 * i + 1, d)
        # --- feed-forward branch:  h2 = h1 + gate_ff * W2 gelu(W1 x2 + b1) ---
        ops.gate_mul(dh, tgf, m2.gate_txt, m2.gate_vid, m2.bs, d, S, St)
        if ff2:
            # h2 = h1 + gate (x) [g | T2] [W2 | s B2]^T, g = gelu(u), T2 = (keep (x) g) A2^T / (1 - p)
            ops.gemm(tgf, Lw.w2_bt, tgf[:, d:], None, K=d)                              # dT2 = tg (s B2)
            _lora_db(st, tn, tgf, a.g[:, dff:], st.view(st.grad, i, "B", 5), d, Lw.c_2 if dora else None)   # dB2 (reads the saved T2: no mask)
            if dora:
                _dora_dm(st, i, 5, tgf[:, :d], a.fo, Lw.b2)
            _lora_da(st, i, "ff2", a.g, None, dff, drop, dt0=tgf[:, d:])                # dA2
            if drop is None:        # du = gelu'(u) (x) (tg W2 + dT2 A2): the correction rides in the K-extension, under the dGELU epilogue
                ops.gemm(tgf, Lw.w2_t, du, None, epilogue=EPI_DGELU, pre_act_in=a.u, K=d + ef)
            else:                   # the mask sits between dT2 A2 and the GELU: the base product, then the dgelu form of the dX correction
                ops.gemm(tgf, Lw.w2_t, du, None, epilogue=EPI_DGELU, pre_act_in=a.u, K=d)
                _lora_dx_dgelu(st, i, du, tgf[:, d:], a.u, dff, drop)
        else:
            ops.gemm(tg, Lw.w2_t, du, None, epilogue=EPI_DGELU, pre_act_in=a.u)
        ops.gemm(du, Lw.w1_t, dx2, None, tile=ops.gemm_block_tile(M, Lw.w1_t.shape[0], dff))   # ff.net.0.proj adapted: [M, d+ext]: dx2 | dT1
        if ff1:
            _lora_db(st, tn, du, a.x2[:, d:], st.view(st.grad, i, "B", 4), dff, Lw.c_1 if dora else None)  # dB1
            if dora:
                _dora_dm(st, i, 4, du, a.u, Lw.b1)
            _lora_da(st, i, "ff1", a.x2, dx2, d, drop)                                  # dA1
            _lora_dx(st, i, "ff1", dx2, d, drop)
        ops.ln_modulate_bwd(dx2, a.h1, a.mean2, a.rstd2, Lw.n2g, (m2.scale_txt, m2.scale_vid, m2.bs), dh, dh1, d, S, St)
        # --- attention branch:  h1 = h + gate_msa * (Wo' [O | T2]) ---
        ops.gate_mul(dh1, tg, m1.gate_txt, m1.gate_vid, m1.bs, d, S, St)
        ops.gemm(tg, Lw.w_o_t, dO, None)                                  # [M, d+ext_o]: dO | dT2
        out_adapted = dora and "to_out.0" in st.targets
        _lora_db(st, tn, tg, a.o[:, d:], st.b_out(st.grad, i), d, Lw.c_o if out_adapted else None)   # dB_o (reads the saved T: no mask)
        if out_adapted:
            _dora_dm(st, i, 3, tg, a.ao, Lw.b_o)
        _lora_da(st, i, "out", a.o, dO, d, drop)                                    # dA_o
        _lora_dx(st, i, "out", dO, d, drop)
        dq.zero_()
        qk3, qkv3 = a.qkh.view(B, S, 2 * d), a.qkv.view(B, S, 3 * d)
        ops.attn_bwd(qk3[:, :, :d], qk3[:, :, d:], qkv3[:, :, 2 * d:], a.o.view(B, S, d + eo)[:, :, :d],
                     dO.view(B, S, d + eo)[:, :, :d], a.lse, delta, dq, dkh.view(B, S, d),
                     dqkv.view(B, S, 3 * d)[:, :, 2 * d:], B, H, S, q_prescaled=True, chain_ws=chain_ws)
        ops.qk_layernorm_bwd(dq.view(M, d), dkh, a.qkv, a.qmean, a.qrstd, Lw.gq, Lw.gk, dqkv, H, rope=ctx.rope)
        if i > 0:
            ops.gemm(dqkv, Lw.w_qkv_t, dx1, None)                         # [M, d+ext_qkv]: dx1 | dT1
        else:
            ops.gemm(dqkv, Lw.w_qkv_t[d:], dx1[:, d:], None)              # the first block's input (frozen embeddings) needs no gradient: dT1 only
        qkv_adapted = dora and any(t in st.targets for t in TARGETS[:3])
        _lora_db(st, tn, dqkv, a.x1[:, d:], st.b_qkv(st.grad, i), d, Lw.c_qkv if qkv_adapted else None)
        if qkv_adapted:
            _dora_dm(st, i, 0, dqkv, a.qkv, Lw.b_qkv, n=3)
        _lora_da(st, i, "qkv", a.x1, dx1, d, drop)
        if i > 0:
            _lora_dx(st, i, "qkv", dx1, d, drop)
            ops.ln_modulate_bwd(dx1, a.h_in, a.mean1, a.rstd1, Lw.n1g, (m1.scale_txt, m1.scale_vid, m1.bs), dh1, dh_in,
                                d, S, St)
            dh, dh_in = dh_in, dh
        ctx.blocks[i] = None        # release this block's activations
    return None


class _DiTFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, x, text, t, rope):
        out, saved = run_forward(model, x, text, t, save=True, rope=rope)
        ctx.model, ctx.saved = model, saved
        return out

    @staticmethod
    def backward(ctx, dout):
        if getattr(ctx.model, "fullft", None) is not None:
            from .engine_fullft import run_backward_fullft
            run_backward_fullft(ctx.model, ctx.saved, dout.contiguous(), ctx.model.fullft.on_grads_ready)
        else:
            run_backward(ctx.model, ctx.saved, dout.contiguous())
        ctx.saved = None
        return None, None, None, None, None, None


def _rope_tables(model, image_rotary_emb, Sv: int, dev):
    """(cos, sin) as handed over by the workflow (cogvideo_pl.py:846-859) -> contiguous fp32 [Sv, 64] on the device"""
    if image_rotary_emb is None:
        return None
    cos, sin = image_rotary_emb
    out = []
    for tb in (cos, sin):
        if tuple(tb.shape) != (Sv, model.config.attention_head_dim):
            raise ValueError(f"image_rotary_emb tables must be [{Sv}, {model.config.attention_head_dim}], got {tuple(tb.shape)}")
        out.append(tb.detach().to(device=dev, dtype=torch.float32).contiguous())
    return out[0], out[1]


def dit_apply(model, hidden_states, encoder_hidden_states, timestep, image_rotary_emb=None):
    x = hidden_states
    if x.dtype != BF16:
        raise TypeError(f"hidden_states must be bf16 (model dtype), got {x.dtype}")
    x = x.contiguous()
    text = encoder_hidden_states
    if text.dtype == torch.float32:
        tb = torch.empty(text.shape, dtype=BF16, device=text.device)
        ops.cast_f32_bf16(text.contiguous(), tb)
        text = tb
    text = text.contiguous()
    if timestep.dim() == 0:
        timestep = timestep[None].expand(x.shape[0])
    t = timestep.to(torch.int64).contiguous()
    st = model.lora
    need_grad = torch.is_grad_enabled() and ((st is not None and any(p.requires_grad for p in st.params))
                                             or getattr(model, "fullft", None) is not None)
    p = model.config.patch_size
    rope = _rope_tables(model, image_rotary_emb, x.shape[1] * (x.shape[3] // p) * (x.shape[4] // p), x.device)
    if not need_grad:
        out, _ = run_forward(model, x, text, t, save=False, rope=rope)
        return out
    anchor = torch.zeros(1, device=x.device, requires_grad=True)
    return _DiTFn.apply(anchor, model, x, text, t, rope)
