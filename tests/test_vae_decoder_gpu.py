"""CogVideoX VAE decoder on the device: vt_spatialnorm_silu_cl and vt_upsample_conv2d_cl against fp32 torch on the bf16-rounded operands
(tiny odd shapes, then the decoder's real last level to cross the 2 GiB / 4 GiB offsets), the whole decoder against the CPU restatement
with a bar from the restatement's own bf16 noise floor, the workflow hook and the real configuration.  The inputs and bars of the small
cases come from tests/vae_decoder_ref.py; tests/test_vae_decoder_cpu.py shows on the CPU that they separate every listed wrong kernel."""
import pytest
import torch
import torch.nn.functional as F

import vae_decoder_ref as R
from parity import cosine, poisoned, untouched

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def _cl(x, dev, pad=0):
    """[N, C, T, H, W] fp32 (bf16-representable) -> channels-last bf16 [N, T, H, W, C] on the device; pad > 0: a view of a poisoned buffer
    with C + pad channels per position (a strided ldx)"""
    x = x.permute(0, 2, 3, 4, 1).to(BF16)
    if not pad:
        return x.contiguous().to(dev)
    buf = poisoned(tuple(x.shape[:4]) + (x.shape[4] + pad,), BF16, dev)
    buf[..., :x.shape[4]] = x.to(dev)
    return buf[..., :x.shape[4]]


def _within(got, ref, bar, what):
    """every element within its own bar; NaN / Inf on the device side are out of tolerance"""
    where = got.device                                            # the large frames are compared where they are
    got, ref, bar = got.double(), ref.to(where).double(), bar.to(where).double()
    assert bool(torch.isfinite(ref).all()) and got.shape == ref.shape, what
    err = (got - ref).abs()
    ok = err <= bar
    worst = (err / bar.clamp_min(1e-300))[torch.isfinite(err)].max().item() if bool(torch.isfinite(err).any()) else float("nan")
    print(f"{what}: worst error / bar {worst:.3f}")
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} of {ok.numel()} elements out of their bar (worst error / bar {worst:.3g}), " \
                           f"{int((~torch.isfinite(got)).sum())} non-finite"


# ------------------------------------------------------------------ vt_spatialnorm_silu_cl
@pytest.mark.parametrize("case", R.spn_cases(), ids=lambda c: "C%d-Tz%d-T%d-r%d" % c)
def test_spatialnorm_silu(dev, case):
    from vt355 import ops
    C, Tz, T, ratio = case
    I = R.spn_inputs(case)
    mod = _cl(torch.cat([I["mod_y"], I["mod_b"]], dim=1), dev)
    gamma, beta = I["gamma"].to(BF16).to(dev), I["beta"].to(BF16).to(dev)
    for silu, strided in R.SPN_VARIANTS:
        x = _cl(I["x"], dev, pad=8 if strided else 0)
        N, T_, H, W, _ = x.shape
        ybuf = poisoned((N, T_, H, W, C + (16 if strided else 0)), BF16, dev)
        y = ybuf[..., :C]
        ops.spatialnorm_silu(x, gamma, beta, mod, y, silu=silu)
        ref, bar = R.spatial_norm3d_table(I["x"], I["mod_y"], I["mod_b"], I["gamma"], I["beta"], silu)
        _within(y.permute(0, 4, 1, 2, 3).float(), ref, bar, f"spatialnorm {case} silu={silu} strided={strided}")
        untouched(ybuf, (Ellipsis, slice(0, C)), "spatialnorm y")


def test_spatialnorm_refuses_other_ratios(dev):
    from vt355 import ops
    x = torch.zeros(1, 5, 6, 4, 64, dtype=BF16, device=dev)
    # H / Hz = 1.5;  W / Wz = 4 / 3;  (T - 1) / (Tz - 1) = 4 / 3;  T > 1 on a one-frame latent
    for zshape in ((1, 2, 4, 4, 128), (1, 2, 6, 3, 128), (1, 4, 6, 4, 128), (1, 1, 6, 4, 128)):
        mod = torch.zeros(zshape, dtype=BF16, device=dev)
        with pytest.raises(ValueError):
            ops.spatialnorm_silu(x, None, None, mod, poisoned(tuple(x.shape), BF16, dev))


# ------------------------------------------------------------------ vt_upsample_conv2d_cl
@pytest.mark.parametrize("case", R.up_cases(), ids=lambda c: "C%d-T%d-t%d" % c)
def test_upsample_conv2d(dev, case):
    from vt355 import ops
    C, T, tup = case
    I = R.up_inputs(case)
    x = _cl(I["x"], dev)
    wk = ops.pack_conv_weight(I["w"].to(BF16).to(dev))
    ref = R.upsample3d(I["x"], I["w"], I["b"], tup)
    bar = R.upsample3d_bar(I["x"], I["w"], tup, ref)
    N, _, To, Ho, Wo = ref.shape
    assert (To, Ho, Wo) == (1 + 2 * (T - 1) if tup and T > 1 else T, 10, 14)
    y = poisoned((N, To, Ho, Wo, C), BF16, dev)
    ops.upsample_conv2d(x, wk, I["b"].to(BF16).to(dev), y, tup)
    _within(y.permute(0, 4, 1, 2, 3).float(), ref, bar, f"upsample_conv2d {case}")


# ------------------------------------------------------------------ the decoder's real last level: offsets past 2 GiB and 4 GiB
_FRAME_BYTES = 480 * 720 * 256 * 2


def _straddlers(frames):
    """frames 0, 1, the frames whose bytes contain the 2 GiB and 4 GiB offsets (where the tensor reaches them), and the last"""
    pick = {0, 1, frames - 1}
    for lim in (1 << 31, 1 << 32):
        if lim < frames * _FRAME_BYTES:
            pick.add(lim // _FRAME_BYTES)
    return sorted(pick)


def _randn_bf16(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    out = poisoned(tuple(shape), BF16, dev)
    for i in range(shape[0]):                                     # frame by frame: no fp32 copy of the whole tensor
        out[i] = (scale * torch.randn(shape[1:], generator=g, device=dev)).to(BF16)
    return out


def _conv3x3_cl(up, w, b):
    """up [H, W, Cin] fp32, w [Cout, Cin, 3, 3] fp32 -> [H, W, Cout]: the 3x3 convolution with zero padding 1 as nine shifted fp32 matrix
    products (plain torch on the device; no convolution library has to pick or build a kernel for a 480 x 720 x 256 fp32 frame)"""
    H, W, C = up.shape
    p = F.pad(up, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(H * W, w.shape[0], dtype=torch.float32, device=up.device) if b is None else b.expand(H * W, -1).clone()
    for dh in range(3):
        for dw in range(3):
            out.addmm_(p[dh:dh + H, dw:dw + W].reshape(H * W, C), w[:, :, dh, dw].t())
    return out.view(H, W, -1)


@pytest.mark.parametrize("T,temporal", [(13, True), (49, False)], ids=["13to25", "49"])
def test_upsample_conv2d_last_level_offsets(dev, T, temporal):
    """C = 256, 240 x 360 -> 480 x 720.  13 -> 25 frames (4.4 GB of output): the frames at the 2 GiB and 4 GiB output offsets, the first
    two and the last.  49 frames, no temporal upsampling (the decoder's real last Upsample3D: 2.2 GB in, 8.7 GB out): the same frames, and
    the last one reads the input past 2 GiB and is stored past 8 GiB"""
    from vt355 import ops
    C, H, W = 256, 240, 360
    x = _randn_bf16((T, H, W, C), dev, 41).view(1, T, H, W, C)
    w = (torch.randn(C, C, 3, 3, generator=torch.Generator().manual_seed(42)) / (9 * C) ** 0.5).to(BF16).to(dev)
    b = (0.1 * torch.randn(C, generator=torch.Generator().manual_seed(43))).to(BF16).to(dev)
    To = 1 + 2 * (T - 1) if temporal else T
    assert To * _FRAME_BYTES > (1 << 32)
    y = poisoned((1, To, 2 * H, 2 * W, C), BF16, dev)
    ops.upsample_conv2d(x, ops.pack_conv_weight(w), b, y, temporal)
    frames = _straddlers(To)
    assert frames == [0, 1, 12, 24, To - 1][:len(frames)] and (T == 13 or x.numel() * 2 > (1 << 31) and To * _FRAME_BYTES > (1 << 33))
    src = R.upsample_nearest(torch.arange(T, dtype=torch.float32).view(1, 1, T, 1, 1), temporal).long().flatten().tolist()[::4]   # F.interpolate's frame map
    assert len(src) == To
    for t in frames:
        xf = x[0, src[t]].permute(2, 0, 1).float().unsqueeze(0)                                # [1, C, H, W] over channels-last memory
        up = F.interpolate(xf, scale_factor=2.0, mode="nearest").permute(0, 2, 3, 1)[0].contiguous()       # [2H, 2W, C]
        ref = _conv3x3_cl(up, w.float(), b.float())
        bar = 2.0 ** -8 * ref.abs() + 2.0 ** -16 * _conv3x3_cl(up.abs(), w.float().abs(), None)
        _within(y[0, t].float(), ref, bar, f"upsample_conv2d last level T={T}, frame {t}")


def test_spatialnorm_silu_last_level_offsets(dev):
    """x of 256 channels x 13 frames x 480 x 720 (2.3 GB): frames 0, 1 and the last, which holds the 2 GiB offset"""
    from vt355 import ops
    C, T, H, W, Tz, Hz, Wz = 256, 13, 480, 720, 4, 60, 90
    x = _randn_bf16((T, H, W, C), dev, 51).view(1, T, H, W, C)
    x += (0.5 * torch.randn(C, generator=torch.Generator().manual_seed(52))).to(BF16).to(dev)
    g = torch.Generator().manual_seed(53)
    mod = torch.cat([1.0 + 0.5 * torch.randn(1, Tz, Hz, Wz, C, generator=g), 0.5 * torch.randn(1, Tz, Hz, Wz, C, generator=g)], dim=-1).to(BF16).to(dev)
    gamma = (1.0 + 0.2 * torch.randn(C, generator=g)).to(BF16).to(dev)
    beta = (0.3 * torch.randn(C, generator=g)).to(BF16).to(dev)
    y = poisoned((1, T, H, W, C), BF16, dev)
    ops.spatialnorm_silu(x, gamma, beta, mod, y, silu=True)
    frames = _straddlers(T)
    assert frames == [0, 1, 12] and T * _FRAME_BYTES > (1 << 31)
    # whole-clip statistics in fp64 from per-frame fp32 sums about zero (|mean| ~ 0.5, std ~ 1: no cancellation to speak of)
    s = torch.zeros(32, dtype=torch.float64, device=dev); q = torch.zeros_like(s)
    for t in range(T):
        xf = x[0, t].float().view(-1, 32, C // 32)
        s += xf.sum(dim=(0, 2), dtype=torch.float64); q += (xf * xf).sum(dim=(0, 2), dtype=torch.float64)
    cnt = T * H * W * (C // 32)
    mean = s / cnt
    rstd = 1.0 / torch.sqrt(q / cnt - mean * mean + 1e-6)
    mean_c, rstd_c = mean.repeat_interleave(C // 32).float(), rstd.repeat_interleave(C // 32).float()
    tz = R.interp_zq(torch.arange(Tz, dtype=torch.float32).view(1, 1, Tz, 1, 1), (T, 1, 1)).long().flatten().tolist()     # F.interpolate's frame map
    for t in frames:
        tab = F.interpolate(mod[0, tz[t]].permute(2, 0, 1).float().unsqueeze(0), size=(H, W), mode="nearest")[0]      # [2C, H, W]
        nf = (x[0, t].float() - mean_c) * rstd_c * gamma.float() + beta.float()                                        # [H, W, C]
        Y, Bm = tab[:C].permute(1, 2, 0), tab[C:].permute(1, 2, 0)
        ref = F.silu(nf * Y + Bm)
        bar = 2.0 ** -7 * ((nf * Y).abs() + Bm.abs())
        _within(y[0, t].float(), ref, bar, f"spatialnorm last level, frame {t}")


# ------------------------------------------------------------------ the whole decoder against the restatement
def _module(P, dev):
    from vt355.vae import CogVideoXVaeDecoder
    c = R.DEC_CFG
    m = CogVideoXVaeDecoder(ch=c.ch, ch_mult=c.ch_mult, num_res_blocks=c.num_res_blocks, z_channels=c.z_channels,
                            temporal_compress_times=c.temporal_compress_times)
    m.load_state_dict(P, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("shape", R.DEC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decoder_against_ref(dev, shape):
    """bar = 3 x the restatement's own bf16 noise floor (max-normalised error of its store_dtype=bfloat16 run against its fp32 run; the 3
    covers MFMA accumulation order and atomic statistics, which the rounding model does not include), and cosine > 0.999.
    Measured on an MI355X (bf16 floor / device error, max-normalised): 3x2x3 7.6e-3 / 9.1e-3, 1x2x3 8.4e-3 / 9.1e-3, 2x3x2 6.4e-3 / 7.5e-3:
    1.1 .. 1.2 x the floor, cosine 0.99997."""
    P, z = R.decoder_inputs(shape)
    ref = R.decoder_forward(P, R.DEC_CFG, z)
    floor = R.max_norm_err(R.decoder_forward(P, R.DEC_CFG, z, store_dtype=BF16), ref)
    out = _module(P, dev)(z)
    T, H, W = shape
    assert out.dtype == BF16 and tuple(out.shape) == (2, 3, 1 + 4 * (T - 1), 4 * H, 4 * W) == tuple(ref.shape)
    got = out.float().cpu()
    assert bool(torch.isfinite(got).all())
    err, cos = R.max_norm_err(got, ref), cosine(got, ref)
    print(f"decoder {shape}: bf16 floor {floor:.3e}, device error {err:.3e} ({err / floor:.2f} x the floor), cosine {cos:.6f}")
    assert 0 < floor < 0.1
    assert err <= 3 * floor and cos > 0.999, (err, floor, cos)


def test_decoder_refuses_wrong_input(dev):
    P, z = R.decoder_inputs(R.DEC_SHAPES[1])
    m = _module(P, dev)
    with pytest.raises(ValueError):
        m(z[:, :3])
    assert tuple(m.decode(z).sample.shape) == (2, 3, 1, 8, 12)


# ------------------------------------------------------------------ workflow hook, real configuration
def test_workflow_decode_latents(dev, tmp_path, monkeypatch):
    from vt355.config import instantiate_from_config
    vcfg = dict(ch=64, ch_mult=[1, 2, 2, 4], num_res_blocks=1, z_channels=4, temporal_compress_times=4, scaling_factor=0.7)
    node = R.make_workflow_dir(tmp_path, with_decoder=True, vcfg=vcfg)
    monkeypatch.chdir(tmp_path)
    wf = instantiate_from_config(node)
    wf.model.to(dev)
    lat = torch.randn(1, 3, 4, 4, 6, generator=torch.Generator().manual_seed(5)).to(dev)       # [B, F, C, H, W]
    dec = wf._decoder()
    assert dec.device.type == "cuda" and wf.vae_decoder is dec
    seen = []
    fwd = dec.forward
    monkeypatch.setattr(dec, "forward", lambda z: (seen.append(z), fwd(z))[1])
    frames = wf.decode_latents(lat)
    assert frames.dtype == BF16 and tuple(frames.shape) == (1, 3, 9, 32, 48) and bool(torch.isfinite(frames.float()).all())
    z = (1 / 0.7 * lat.permute(0, 2, 1, 3, 4)).to(BF16)
    assert len(seen) == 1 and torch.equal(seen[0], z)            # exactly the permuted latent / scaling_factor reached the decoder
    # "equals decoder(z / scaling_factor)": a second decode of the same z is not bit-identical (the GroupNorm sums are fp32 atomics, their
    # order is free), so both are held to the decoder test's bar against the restatement run on this checkpoint's weights
    cfg = R.VaeDecConfig(ch=64, ch_mult=(1, 2, 2, 4), num_res_blocks=1, z_channels=4, temporal_compress_times=4)
    P = {k: v.float().cpu() for k, v in dec.state_dict().items()}
    ref = R.decoder_forward(P, cfg, z.float().cpu())
    floor = R.max_norm_err(R.decoder_forward(P, cfg, z.float().cpu(), store_dtype=BF16), ref)
    for got in (frames, fwd(z)):
        err = R.max_norm_err(got.float().cpu(), ref)
        print(f"decode_latents: bf16 floor {floor:.3e}, device error {err:.3e}")
        assert 0 < floor < 0.1 and err <= 3 * floor and cosine(got, ref) > 0.999
    first = wf.decode_first_stage(lat.permute(0, 2, 1, 3, 4))
    assert len(seen) == 2 and torch.equal(seen[1].to(BF16), z) and tuple(first.sample.shape) == (1, 3, 9, 32, 48)


def test_decoder_real_configuration(dev):
    """CogVideoX's decoder (128, (1, 2, 2, 4), 3) on a 13 x 60 x 90 latent: 49 x 480 x 720 frames, every activation size of a real decode"""
    from vt355.vae import CogVideoXVaeDecoder
    m = CogVideoXVaeDecoder().init_weights(1).to(dev)
    z = torch.randn(1, 16, 13, 60, 90, generator=torch.Generator().manual_seed(6))
    out = m(z)
    assert out.dtype == BF16 and tuple(out.shape) == (1, 3, 49, 480, 720)
    assert bool(torch.isfinite(out.float()).all()) and float(out.float().abs().max()) > 0
