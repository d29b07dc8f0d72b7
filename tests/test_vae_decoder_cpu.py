"""CogVideoX VAE decoder, everything that runs without a GPU: the CPU restatement (tests/vae_decoder_ref.py) against the twin's goldens,
the module's names / loaders / refusals, the kernels' integer index rules against F.interpolate, the mutants against the GPU tests' own
inputs and bars, the workflow hooks, the header."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import golden_io
import vae_decoder_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _t(a):
    return torch.from_numpy(a)


# ------------------------------------------------------------------ 1. the restatement equals the twin
def test_ref_equals_decoder_golden():
    g = golden_io.load("vae_decoder_tiny")
    P = {k[2:]: _t(g[k]) for k in g.files if k.startswith("P.")}
    cfg = R.tiny_config()
    for zk, ok in (("z", "out"), ("z1", "out1")):
        out = R.decoder_forward(P, cfg, _t(g[zk]))
        want = _t(g[ok])
        assert out.shape == want.shape
        assert R.max_norm_err(out, want) <= 1e-5, (zk, R.max_norm_err(out, want))
    assert tuple(g["out"].shape) == (1, 3, 9, 16, 24) and tuple(g["out1"].shape) == (1, 3, 1, 16, 24)


def test_ref_equals_upsample3d_golden():
    g = golden_io.load("vae_upsample3d")
    for ct in (0, 1):
        w, b = _t(g[f"ct{ct}.conv.weight"]), _t(g[f"ct{ct}.conv.bias"])
        for T in (1, 2, 3):
            y = R.upsample3d(_t(g[f"ct{ct}.x{T}"]), w, b, bool(ct))
            want = _t(g[f"ct{ct}.y{T}"])
            assert y.shape == want.shape and want.shape[2] == (1 + 2 * (T - 1) if ct and T > 1 else T)
            assert R.max_norm_err(y, want) <= 1e-5, (ct, T)


def test_ref_equals_spatialnorm3d_golden():
    g = golden_io.load("vae_spatialnorm3d")
    P = {k[2:]: _t(g[k]) for k in g.files if k.startswith("P.")}
    tags = sorted(k[:-4] for k in g.files if k.endswith(".out"))
    assert len(tags) == 6
    for tag in tags:
        f, zq, want = _t(g[tag + ".f"]), _t(g[tag + ".zq"]), _t(g[tag + ".out"])
        out = R.spatial_norm3d(f, zq, P["norm_layer.weight"], P["norm_layer.bias"], P["conv_y.conv.weight"], P["conv_y.conv.bias"],
                               P["conv_b.conv.weight"], P["conv_b.conv.bias"])
        assert R.max_norm_err(out, want) <= 1e-5, tag
        # the device's order -- the 1x1x1 convolutions at latent resolution, then the gather -- is the same function
        my = R.causal_conv3d(zq, P["conv_y.conv.weight"], P["conv_y.conv.bias"])
        mb = R.causal_conv3d(zq, P["conv_b.conv.weight"], P["conv_b.conv.bias"])
        out2, _ = R.spatial_norm3d_table(f, my, mb, P["norm_layer.weight"], P["norm_layer.bias"])
        assert R.max_norm_err(out2, want) <= 1e-5, tag


# ------------------------------------------------------------------ 2. the module: names, loaders, refusals
def _tiny_module():
    from vt355.vae import CogVideoXVaeDecoder
    cfg = R.tiny_config()
    return CogVideoXVaeDecoder(ch=cfg.ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks, z_channels=cfg.z_channels,
                               temporal_compress_times=cfg.temporal_compress_times)


def test_module_names_and_shapes_are_the_twins():
    g = golden_io.load("vae_decoder_tiny")
    want = {k[2:]: tuple(g[k].shape) for k in g.files if k.startswith("P.")}      # the twin loaded these with strict=True
    m = _tiny_module()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want, (sorted(set(got) ^ set(want))[:8], [k for k in got if k in want and got[k] != want[k]][:8])
    assert all(v.dtype == BF16 for v in m.state_dict().values())
    m.load_state_dict({k[2:]: _t(g[k]) for k in g.files if k.startswith("P.")}, strict=True)
    assert torch.equal(m.up[1].upsample.conv.weight, _t(g["P.up.1.upsample.conv.weight"]).to(BF16))
    assert m.up[2].upsample.compress_time and m.up[1].upsample.compress_time and not hasattr(m.up[0], "upsample")
    from vt355.vae import CogVideoXVaeDecoder
    full = CogVideoXVaeDecoder()                                                   # CogVideoX: 128, (1, 2, 2, 4), 3 + 1 blocks per level
    assert [len(l.block) for l in full.up] == [4] * 4 and full.conv_in.conv.weight.shape == (512, 16, 3, 3, 3)
    assert [full.up[i].upsample.compress_time for i in (1, 2, 3)] == [False, True, True]
    assert full.up[0].block[0].nin_shortcut.weight.shape == (128, 256, 1, 1, 1) and full.conv_out.conv.weight.shape == (3, 128, 3, 3, 3)


def test_checkpoint_forms(tmp_path):
    from safetensors.torch import save_file
    from vt355.vae import CogVideoXVaeDecoder
    src = _tiny_module().init_weights(3)
    own = {k: v.clone() for k, v in src.state_dict().items()}
    for pre in ("decoder.", "first_stage_model.decoder."):
        ck = {pre + k: v for k, v in own.items()}
        ck[pre.replace("decoder", "encoder") + "conv_in.conv.weight"] = torch.zeros(3)          # other sub-trees are ignored
        ck["loss.logvar"] = torch.zeros(1)
        m = _tiny_module()
        m.load_state_dict(ck)
        assert all(torch.equal(v, own[k]) for k, v in m.state_dict().items())
    with pytest.raises(KeyError, match="diffusers"):
        _tiny_module().load_state_dict({"decoder.up_blocks.0.resnets.0.norm1.norm_layer.weight": torch.zeros(4),
                                        "decoder.conv_in.conv.weight": torch.zeros(4)})
    with pytest.raises(RuntimeError, match=r"decoder\."):
        _tiny_module().load_state_dict({"down.0.block.0.norm1.weight": torch.zeros(4), "conv_in.conv.weight": torch.zeros(4)})
    cfg = R.tiny_config()
    d = tmp_path / "vae"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(ch=cfg.ch, ch_mult=list(cfg.ch_mult), num_res_blocks=cfg.num_res_blocks,
                                                   z_channels=cfg.z_channels, scaling_factor=0.7, double_z=True)))
    save_file({"decoder." + k: v.contiguous() for k, v in own.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    m = CogVideoXVaeDecoder.from_pretrained(pretrained_model_name_or_path=str(tmp_path), subfolder="vae")
    assert m.config.scaling_factor == 0.7 and all(torch.equal(v, own[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("kw", [dict(add_conv=True), dict(attn_resolutions=[16]), dict(conv_shortcut=True), dict(give_pre_end=True)])
def test_unsupported_options_raise(kw):
    from vt355.vae import CogVideoXVaeDecoder
    with pytest.raises(NotImplementedError):
        CogVideoXVaeDecoder(**kw)
    CogVideoXVaeDecoder(ch=64, ch_mult=(1, 2), num_res_blocks=1, add_conv=False, attn_resolutions=[], conv_shortcut=False, give_pre_end=False)


# ------------------------------------------------------------------ 3. the integer index rules are F.interpolate's
@pytest.mark.parametrize("Tz", [1, 2, 3, 13])
def test_zq_index_rule_is_nearest_interpolation(Tz):
    from vt355 import ops
    for rt in (1, 2, 4):
        T = 1 + (Tz - 1) * rt
        if Tz == 1 and rt > 1:
            continue
        for rs in (1, 2, 4, 8):
            Hz, Wz = 3, 5
            H, W = Hz * rs, Wz * rs
            idx = torch.arange(Tz * Hz * Wz, dtype=torch.float32).view(1, 1, Tz, Hz, Wz)
            want = R.interp_zq(idx, (T, H, W)).long()[0, 0]
            tz, hz, wz = ops.spatialnorm_zq_index(T, Tz, H, Hz, W, Wz)
            got = (torch.tensor(tz).view(-1, 1, 1) * Hz + torch.tensor(hz).view(1, -1, 1)) * Wz + torch.tensor(wz).view(1, 1, -1)
            assert torch.equal(got, want), (Tz, T, rs)
    if Tz > 1:                                                   # one output frame reads latent frame 0 (the twin's T == 1 branch)
        tz, _, _ = ops.spatialnorm_zq_index(1, Tz, 4, 2, 4, 2)
        idx = torch.arange(Tz * 4, dtype=torch.float32).view(1, 1, Tz, 2, 2)
        assert tz == [0] and R.interp_zq(idx, (1, 4, 4)).long()[0, 0, 0, 0, 0].item() == 0


def test_zq_index_rule_refuses_other_ratios():
    from vt355 import ops
    for args in ((5, 2, 6, 2, 4, 4), (5, 2, 4, 4, 10, 4), (4, 2, 4, 4, 4, 4), (7, 3, 4, 4, 4, 4), (5, 1, 4, 4, 4, 4), (5, 2, 5, 2, 4, 4)):
        with pytest.raises(ValueError):
            ops.spatialnorm_zq_index(*args)


@pytest.mark.parametrize("temporal", [False, True])
def test_upsample_index_rule_is_nearest_interpolation(temporal):
    from vt355 import ops
    for T in (1, 2, 3, 13):
        H, W = 3, 5
        idx = torch.arange(T * H * W, dtype=torch.float32).view(1, 1, T, H, W)
        want = R.upsample_nearest(idx, temporal).long()[0, 0]
        ts = ops.upsample_src_frames(T, temporal)
        assert len(ts) == want.shape[0] == (1 + 2 * (T - 1) if temporal and T > 1 else T)
        got = (torch.tensor(ts).view(-1, 1, 1) * H + (torch.arange(2 * H) >> 1).view(1, -1, 1)) * W + (torch.arange(2 * W) >> 1).view(1, 1, -1)
        assert torch.equal(got, want), (T, temporal)


# ------------------------------------------------------------------ 4. the GPU tests' inputs and bars separate every mutant
def _excess(mut, ref, bar):
    """max over the elements of |mut - ref| / bar (the GPU test fails an element at 1)"""
    return ((mut - ref).abs() / bar.clamp_min(1e-30)).max().item()


@pytest.mark.parametrize("mutant", R.SPN_MUTANTS)
def test_spatialnorm_inputs_separate_the_mutant(mutant):
    seen = 0
    for case in R.spn_cases():
        C, Tz, T, ratio = case
        if mutant == "zq_first" and (T == 1 or T == Tz):
            continue                                             # the two maps coincide: nothing to tell apart on this shape
        I = R.spn_inputs(case)
        for silu in (True, False):
            ref, bar = R.spatial_norm3d_table(I["x"], I["mod_y"], I["mod_b"], I["gamma"], I["beta"], silu)
            mut, _ = R.spatial_norm3d_table(I["x"], I["mod_y"], I["mod_b"], I["gamma"], I["beta"], silu, mutant)
            assert _excess(mut, ref, bar) > 10.0, (mutant, case, silu, _excess(mut, ref, bar))
            seen += 1
    assert seen >= 12


@pytest.mark.parametrize("mutant", R.UP_MUTANTS)
def test_upsample_inputs_separate_the_mutant(mutant):
    seen = 0
    for case in R.up_cases():
        C, T, tup = case
        if mutant == "up_first" and not (tup and T > 1):
            continue
        I = R.up_inputs(case)
        ref = R.upsample3d(I["x"], I["w"], I["b"], tup)
        bar = R.upsample3d_bar(I["x"], I["w"], tup, ref)
        mut = R.upsample3d(I["x"], I["w"], I["b"], tup, mutant=mutant)
        assert _excess(mut, ref, bar) > 10.0, (mutant, case, _excess(mut, ref, bar))
        seen += 1
    assert seen >= 4


_DEC = {}


def _decoder_runs(shape):
    """(fp32 run, bf16 floor) of the GPU test's decoder case, computed once"""
    if shape not in _DEC:
        P, z = R.decoder_inputs(shape)
        ref = R.decoder_forward(P, R.DEC_CFG, z)
        floor = R.max_norm_err(R.decoder_forward(P, R.DEC_CFG, z, store_dtype=BF16), ref)
        _DEC[shape] = (P, z, ref, floor)
    return _DEC[shape]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_decoder_inputs_separate_the_mutant(mutant):
    """the whole-decoder GPU test accepts 3 x the bf16 floor (max-normalised): every mutant is more than 10 x that away on every latent
    shape where it changes anything (a one-frame latent has no first frame to mishandle)"""
    seen = 0
    for shape in R.DEC_SHAPES:
        if mutant in ("zq_first", "up_first") and shape[0] == 1:
            continue
        P, z, ref, floor = _decoder_runs(shape)
        err = R.max_norm_err(R.decoder_forward(P, R.DEC_CFG, z, mutant=mutant), ref)
        print(f"{mutant} {shape}: mutant {err:.3e}, floor {floor:.3e}, ratio to the bar {err / (3 * floor):.1f}")
        assert 0 < floor < 0.1 and err > 10 * 3 * floor, (mutant, shape, err, floor)
        seen += 1
    assert seen >= 2


# ------------------------------------------------------------------ 5. workflow hooks
_workflow_dir = R.make_workflow_dir


def test_workflow_without_decoder_weights(tmp_path, monkeypatch):
    """an encoder-only VAE directory: the constructor behaves as before (encoder loaded, no decoder built), decoding raises by name"""
    from vt355.config import instantiate_from_config
    node = _workflow_dir(tmp_path, with_decoder=False)
    monkeypatch.chdir(tmp_path)
    wf = instantiate_from_config(node)
    assert wf.vae.config.scaling_factor == 0.7 and callable(wf.first_stage)
    assert not any("decoder" in k for k in wf.state_dict()) and not hasattr(wf, "vae_decoder")
    for call in (lambda: wf.decode_latents(torch.zeros(1, 2, 16, 2, 2)), lambda: wf.decode_first_stage(torch.zeros(1, 16, 2, 2, 2))):
        with pytest.raises(RuntimeError, match=r"decoder\."):
            call()
    assert not hasattr(wf, "vae_decoder") and not hasattr(wf, "log_images")


def test_workflow_builds_the_decoder_lazily(tmp_path, monkeypatch):
    from vt355.config import instantiate_from_config
    from vt355.vae import CogVideoXVaeDecoder
    node = _workflow_dir(tmp_path, with_decoder=True)
    monkeypatch.chdir(tmp_path)
    wf = instantiate_from_config(node)
    assert callable(wf.first_stage) and not hasattr(wf, "vae_decoder")         # `encoder.` sub-tree loaded, nothing else built yet
    dec = wf._decoder()
    assert isinstance(dec, CogVideoXVaeDecoder) and dec.config.scaling_factor == 0.7 and wf._decoder() is dec
    from vt355.workflow import CogVideoXWorkFlow
    wf2 = CogVideoXWorkFlow.__new__(CogVideoXWorkFlow)
    torch.nn.Module.__init__(wf2)
    wf2._first_stage_config = None                               # explicit first_stage callables, no config node
    wf2.model = torch.nn.Linear(1, 1)
    with pytest.raises(RuntimeError, match=r"decoder\."):
        wf2.decode_latents(torch.zeros(1, 2, 16, 2, 2))


# ------------------------------------------------------------------ 6. header and exports
def test_symbols_declared_and_exported():
    import vt355
    from vt355._lib import PROTOTYPES
    header = open(os.path.join(ROOT, "include", "vt355.h")).read()
    assert "currently 2" in header                               # new symbols only: the ABI version stays
    lib = vt355.load_library()
    for name, nargs in (("vt_spatialnorm_silu_cl", 21), ("vt_upsample_conv2d_cl", 14)):
        assert f"int {name}(" in header and len(PROTOTYPES[name]) == nargs and hasattr(lib, name), name
    at = header.index("int vt_spatialnorm_silu_cl(")
    assert "Replaces:" in header[header.rindex("/*", 0, at):at]
    at = header.index("int vt_upsample_conv2d_cl(")
    assert "Replaces:" in header[header.rindex("/*", 0, at):at]
    import inspect
    from vt355 import vae
    assert "decoder is not built" not in inspect.getdoc(vae)
