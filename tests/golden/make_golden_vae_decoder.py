#!/usr/bin/env python3
"""Generates tests/golden/vae_decoder_tiny*.npz, vae_upsample3d.npz and vae_spatialnorm3d.npz (tests/golden_io.py) by running the
reference's own ContextParallelDecoder3D / Upsample3D / SpatialNorm3D (videotuna/models/cogvideo_sat/vae_modules/cp_enc_dec.py) on
seeded weights in the build container, with the stubs of make_golden_vae.py (beartype, sgm.util's context-parallel getters -> world 1 /
rank 0, vae_modules.utils.SafeConv3d -> torch.nn.Conv3d; a 1-rank gloo group serves torch.distributed.get_rank()).
Run:  python tests/golden/make_golden_vae_decoder.py   (needs /root/reference; the .npz files it writes are what travels)"""
import importlib.util
import os
import sys
import types
import typing

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, ".."))
import golden_io  # noqa: E402  (fixtures of more than 1 MiB are stored in parts)
import vae_decoder_ref as R  # noqa: E402


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def main():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29534")
    dist.init_process_group("gloo", rank=0, world_size=1)
    stub("beartype", beartype=lambda f: f)
    stub("beartype.typing", **{k: getattr(typing, k) for k in ("List", "Optional", "Tuple", "Union")})
    stub("sgm")
    stub("sgm.util", get_context_parallel_group=lambda: None, get_context_parallel_group_rank=lambda: 0,
         get_context_parallel_rank=lambda: 0, get_context_parallel_world_size=lambda: 1)
    stub("vae_modules")
    stub("vae_modules.utils", SafeConv3d=torch.nn.Conv3d)
    spec = importlib.util.spec_from_file_location("cp_enc_dec", os.path.join(REF, "videotuna/models/cogvideo_sat/vae_modules/cp_enc_dec.py"))
    mod = importlib.util.module_from_spec(spec); sys.modules["cp_enc_dec"] = mod
    spec.loader.exec_module(mod)

    # ---- the whole decoder: 3 latent frames -> 9 frames, 4x6 -> 16x24; and a one-frame latent (every temporal branch skipped)
    cfg = R.tiny_config()
    dec = mod.ContextParallelDecoder3D(ch=cfg.ch, out_ch=cfg.out_ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks, attn_resolutions=[],
                                       in_channels=3, resolution=16, z_channels=cfg.z_channels,
                                       temporal_compress_times=cfg.temporal_compress_times).eval()
    P = R.init_params(cfg, seed=5)
    dec.load_state_dict(P, strict=True)
    g = torch.Generator().manual_seed(12)
    z = torch.randn(1, cfg.z_channels, 3, 4, 6, generator=g)
    z1 = torch.randn(1, cfg.z_channels, 1, 4, 6, generator=g)
    with torch.no_grad():
        out, out1 = dec(z), dec(z1)
    golden_io.save(os.path.join(HERE, "vae_decoder_tiny.npz"), z=z.numpy(), out=out.numpy(), z1=z1.numpy(), out1=out1.numpy(),
                   **{"P." + k: v.numpy() for k, v in P.items()})
    print("wrote vae_decoder_tiny", tuple(out.shape), tuple(out1.shape), float(out.abs().max()))

    # ---- Upsample3D alone: compress_time on and off, T in {1, 2, 3}
    gu = torch.Generator().manual_seed(13)
    rec = {}
    for ct in (False, True):
        up = mod.Upsample3D(64, with_conv=True, compress_time=ct).eval()
        with torch.no_grad():
            for p_ in up.parameters():
                p_.copy_(torch.randn(p_.shape, generator=gu) * 0.1)
        rec[f"ct{int(ct)}.conv.weight"] = up.conv.weight.detach().numpy()
        rec[f"ct{int(ct)}.conv.bias"] = up.conv.bias.detach().numpy()
        for T in (1, 2, 3):
            x = torch.randn(1, 64, T, 3, 5, generator=gu)
            rec[f"ct{int(ct)}.x{T}"] = x.numpy()
            with torch.no_grad():
                rec[f"ct{int(ct)}.y{T}"] = up(x).numpy()
    golden_io.save(os.path.join(HERE, "vae_upsample3d.npz"), **rec)
    print("wrote vae_upsample3d", {k: v.shape for k, v in rec.items() if ".y" in k})

    # ---- SpatialNorm3D alone: (T, Tz) in {(1, 1), (5, 2), (1, 2)}, spatial ratios 1 and 4
    gs = torch.Generator().manual_seed(14)
    sn = mod.SpatialNorm3D(64, 4, freeze_norm_layer=False, add_conv=False, num_groups=32, eps=1e-6, affine=True).eval()
    with torch.no_grad():
        for p_ in sn.parameters():
            p_.copy_(torch.randn(p_.shape, generator=gs) * 0.5)
    rec = {"P." + k: v.detach().numpy() for k, v in sn.state_dict().items()}
    for (T, Tz) in ((1, 1), (5, 2), (1, 2)):
        for ratio in (1, 4):
            f = torch.randn(1, 64, T, 2 * ratio, 3 * ratio, generator=gs)
            zq = torch.randn(1, 4, Tz, 2, 3, generator=gs)
            tag = f"T{T}z{Tz}r{ratio}"
            rec[tag + ".f"], rec[tag + ".zq"] = f.numpy(), zq.numpy()
            with torch.no_grad():
                rec[tag + ".out"] = sn(f, zq).numpy()
    golden_io.save(os.path.join(HERE, "vae_spatialnorm3d.npz"), **rec)
    print("wrote vae_spatialnorm3d", [k for k in rec if k.endswith(".out")])
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
