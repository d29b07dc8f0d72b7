"""CPU: the C-ABI library loads and exports every symbol include/vt355.h declares; host logic (config reflection,
LoRA key naming, checkpoint filter, product path refuses to run without the device)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    import vt355
    from vt355._lib import PROTOTYPES
    lib = vt355.load_library()
    header = open(os.path.join(ROOT, "include", "vt355.h")).read()
    declared = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/vt355.h but not exported by libvt355.so"
    assert declared == set(PROTOTYPES), declared ^ set(PROTOTYPES)
    assert lib.vt_version() == 2 and lib.vt_arch() == b"gfx950"
    assert lib.vt_error_string(-1).decode().startswith("bad shape")


def test_attn_bwd_chain_plan_is_a_host_query():
    """it launches nothing and needs no device: without one the persistent grid falls back to its minimum of 8 slots, nothing can chain
    (chain length <= grid / 8 = 1) and the key blocks are swept in generations of 8"""
    from vt355 import ops
    from vt355._lib import VtError
    L, grid, gens = ops.attn_bwd_chain_plan(1, 6, 600)                         # 3 key blocks x 6 heads = 18 items
    assert (L, grid, gens) == ((3, 24, 1) if torch.cuda.is_available() else (1, 8, 3))
    assert ops.attn_bwd_chain_plan(1, 1, 64, have_ws=False) == (1, 8, 1)
    with pytest.raises(VtError, match="vt_attn_bwd_chain_plan"):
        ops.attn_bwd_chain_plan(1, 0, 600)


def test_no_cpu_fallback():
    from vt355 import ops
    from vt355.dit import CogVideoXTransformer3DModel
    a = torch.zeros(4, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        ops.gemm(a, a, torch.zeros(4, 4, dtype=torch.bfloat16))
    m = CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=1, time_embed_dim=64, text_embed_dim=64)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 2, 16, 4, 4, dtype=torch.bfloat16), torch.zeros(1, 4, 64, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.long))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "videotuna-dev_amd")
    for f in os.listdir(pkg):
        if f.endswith(".py"):
            src = open(os.path.join(pkg, f)).read()
            assert "_oracle" not in src and "import oracle" not in src and "selfcheck" not in src, f


def test_reference_yaml_instantiates_through_target_remap():
    """configs/004_cogvideox/cogvideo2b.yaml's nodes (restated inline: the reference tree is absent on the GPU box)."""
    from vt355.config import instantiate_from_config
    from vt355.lora import LoraConfig
    from vt355.scheduler import CogVideoXDPMScheduler
    adapter = {"target": "peft.LoraConfig", "params": {"r": 4, "lora_alpha": 1.0, "init_lora_weights": True,
                                                       "target_modules": ["to_k", "to_q", "to_v", "to_out.0"]}}
    cfg = instantiate_from_config(adapter)
    assert isinstance(cfg, LoraConfig) and cfg.r == 4 and cfg.lora_alpha == 1.0
    with pytest.raises(FileNotFoundError):          # checkpoints/ does not exist offline: loud, not silent
        instantiate_from_config({"target": "diffusers.CogVideoXTransformer3DModel",
                                 "params": {"pretrained_model_name_or_path": "checkpoints/cogvideo/CogVideoX-2b",
                                            "subfolder": "transformer", "load_dtype": "fp16"}})
    s = instantiate_from_config({"target": "diffusers.CogVideoXDPMScheduler", "params": {}})
    assert isinstance(s, CogVideoXDPMScheduler) and s.config.num_train_timesteps == 1000
    with pytest.raises(KeyError):
        instantiate_from_config({"params": {}})


def test_lora_injection_names_and_checkpoint_filter():
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    from vt355.workflow import CogVideoXWorkFlow
    m = CogVideoXTransformer3DModel(num_layers=2, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(0)
    n_base = sum(p.numel() for p in m.parameters())
    m.requires_grad_(False)
    peft = get_peft_model(m, LoraConfig(r=4, lora_alpha=1.0, target_modules=["to_k", "to_q", "to_v", "to_out.0"]))
    tr, al = peft.get_nb_trainable_parameters()
    assert tr == 2 * 4 * 2 * 4 * 128 and al == n_base + tr
    sd = peft.state_dict()
    assert "base_model.model.transformer_blocks.0.attn1.to_q.base_layer.weight" in sd
    assert "base_model.model.transformer_blocks.1.attn1.to_out.0.lora_B.default.weight" in sd
    # peft init: A ~ U(-1/sqrt(d), 1/sqrt(d)), B = 0
    a = sd["base_model.model.transformer_blocks.0.attn1.to_k.lora_A.default.weight"]
    assert a.shape == (4, 128) and a.abs().max() <= 1 / 128 ** 0.5 and a.abs().max() > 0
    assert sd["base_model.model.transformer_blocks.0.attn1.to_k.lora_B.default.weight"].abs().max() == 0
    # LoRA-only checkpoint filter (cogvideo_pl.py:781-787)
    ck = CogVideoXWorkFlow.on_save_checkpoint(None, {"state_dict": {"model." + k: v for k, v in sd.items()}})
    assert len(ck["state_dict"]) == 16 and all("lora" in k for k in ck["state_dict"])
    # adapter parameters are views of one flat buffer and stay so after .to()
    st = peft._lora_state
    peft.to(torch.device("cpu"))
    assert all(p.data_ptr() >= st.flat.data_ptr() and p.data_ptr() < st.flat.data_ptr() + st.flat.numel() * 4 for p in st.params)


def test_hf_key_names_and_shapes():
    import cogvideox_oracle as O
    from vt355.dit import CogVideoXTransformer3DModel
    cfg = O.tiny_config()
    m = CogVideoXTransformer3DModel(num_layers=cfg.num_layers, num_attention_heads=cfg.num_attention_heads,
                                    time_embed_dim=cfg.time_embed_dim, text_embed_dim=cfg.text_embed_dim)
    sd = m.state_dict()
    shapes = O.param_shapes(cfg)
    assert set(sd) == set(shapes)
    for k, s in shapes.items():
        assert tuple(sd[k].shape) == s, k
    n = sum(int(torch.tensor(s).prod()) for s in O.param_shapes(O.DiTConfig()).values())
    assert abs(n - 1.69e9) < 0.02e9


def test_full_finetune_flat_layout():
    """FullFTState re-homes every parameter into one flat buffer: HF names kept, fused groups contiguous, slices cover it."""
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.fullft import enable_full_finetune
    m = CogVideoXTransformer3DModel(num_layers=2, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(0)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    ft = enable_full_finetune(m)
    assert set(ft.names) == set(before) and ft.numel == sum(v.numel() for v in before.values())
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k                                    # values unchanged, names unchanged
    base = ft.flat_bf16.data_ptr()
    for n, p in m.named_parameters():
        off, shp = ft.offsets[n]
        assert p.data_ptr() == base + 2 * off and off % 8 == 0 and p.requires_grad
    d = m.inner_dim
    w = ft.span(ft.flat_bf16, "transformer_blocks.1.attn1.to_q.weight", "transformer_blocks.1.attn1.to_v.weight", (3 * d, d))
    assert torch.equal(w[d:2 * d], m.transformer_blocks[1].attn1.to_k.weight)
    nmod = (12 * 2 + 2) * d
    wa = ft.span(ft.flat_bf16, "transformer_blocks.0.norm1.linear.weight", "norm_out.linear.weight", (nmod, 64))
    assert torch.equal(wa[6 * d:12 * d], m.transformer_blocks[0].norm2.linear.weight)
    assert torch.equal(ft.flat, ft.flat_bf16.float())
    with pytest.raises(RuntimeError):
        m.to(torch.float32)


def test_from_pretrained_reads_hf_layout(tmp_path):
    """HF directory layout (config.json + diffusion_pytorch_model.safetensors with diffusers key names) round-trips through
    from_pretrained / instantiate_from_config -- the loader a session WITH checkpoints/cogvideo/CogVideoX-2b would use."""
    import json
    from safetensors.torch import save_file
    from vt355.config import instantiate_from_config
    from vt355.dit import CogVideoXTransformer3DModel
    cfg = dict(num_layers=2, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64, sample_width=8, sample_height=6,
               sample_frames=5, max_text_seq_length=10, _class_name="CogVideoXTransformer3DModel", _diffusers_version="0.32.2")
    src = CogVideoXTransformer3DModel(**{k: v for k, v in cfg.items() if not k.startswith("_")}).init_weights(5)
    root = tmp_path / "CogVideoX-tiny" / "transformer"
    root.mkdir(parents=True)
    (root / "config.json").write_text(json.dumps(cfg))
    sd = {k: v.contiguous() for k, v in src.state_dict().items()}
    sd["patch_embed.pos_embedding"] = torch.zeros(1, 10 + 24, 128)       # diffusers stores the fixed table: ignored, regenerated
    save_file(sd, str(root / "diffusion_pytorch_model.safetensors"))
    m = instantiate_from_config({"target": "diffusers.CogVideoXTransformer3DModel",
                                 "params": {"pretrained_model_name_or_path": str(tmp_path / "CogVideoX-tiny"),
                                            "subfolder": "transformer", "load_dtype": "fp16"}})
    assert isinstance(m, CogVideoXTransformer3DModel) and m.config.num_layers == 2
    for k, v in src.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    (tmp_path / "sch").mkdir()
    (tmp_path / "sch" / "scheduler_config.json").write_text(json.dumps({"_class_name": "CogVideoXDPMScheduler", "snr_shift_scale": 1.0,
                                                                       "beta_start": 0.00085, "beta_end": 0.012}))
    s = instantiate_from_config({"target": "diffusers.CogVideoXDPMScheduler",
                                 "params": {"pretrained_model_name_or_path": str(tmp_path), "subfolder": "sch"}})
    assert s.config.snr_shift_scale == 1.0


def test_cogvideox_5b_rope_host_side(tmp_path):
    """CogVideoX-5B / 5B-I2V recipes (configs/004_cogvideox/cogvideo5b*.yaml): the workflow's rotary tables
    (cogvideo_pl.py:442-473) against the golden vectors of the reference's in-tree construction, the I2V target remap,
    and the learned-table buffer of the I2V transformer surviving a checkpoint round trip."""
    import json
    import os
    from safetensors.torch import save_file
    from vt355.config import get_obj_from_str
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.rope import get_3d_rotary_pos_embed, get_resize_crop_region_for_grid, prepare_rotary_positional_embeddings
    from vt355.workflow import CogVideoXI2V, CogVideoXWorkFlow
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "rope_3d.npz"))
    cos, sin = get_3d_rotary_pos_embed(64, ((0, 0), (4, 5)), (4, 5), 3)
    assert np.abs(cos.numpy() - gold["small_cos"]).max() < 1e-6 and np.abs(sin.numpy() - gold["small_sin"]).max() < 1e-6
    cos, sin = prepare_rotary_positional_embeddings(480, 720, 13)          # 49x480x720 -> 13 x 30 x 45 tokens
    assert cos.shape == (17550, 64) and cos.dtype == torch.float32
    idx = gold["full_rows_idx"]
    assert np.abs(cos[idx].numpy() - gold["full_cos_rows"]).max() < 5e-6
    assert np.abs(sin[idx].numpy() - gold["full_sin_rows"]).max() < 5e-6
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                      # the base grid (crop starts at 0) is the pinned case: silent
        get_3d_rotary_pos_embed(64, ((0, 0), (30, 45)), (30, 45), 2)
    with pytest.warns(UserWarning, match="parity unpinned"):                # any other aspect ratio: the diffusers grid variant is unverifiable
        get_3d_rotary_pos_embed(64, ((2, 0), (28, 45)), (26, 45), 2)
    crops = np.load(os.path.join(os.path.dirname(__file__), "golden", "crop_region.npz"))
    for src, tgt, reg in zip(crops["src"], crops["tgt"], crops["region"]):
        assert np.array_equal(np.array(get_resize_crop_region_for_grid(tuple(map(int, src)), tuple(map(int, tgt)))), reg)
    assert get_obj_from_str("videotuna.models.cogvideo_hf.cogvideo_i2v.CogVideoXI2V") is CogVideoXI2V
    assert issubclass(CogVideoXI2V, CogVideoXWorkFlow)
    # 5B-I2V transformer layout: rotary q/k, learned table kept as a persistent buffer, 32 input / 16 output channels
    cfg = dict(num_layers=1, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64, sample_width=8, sample_height=6,
               sample_frames=5, max_text_seq_length=10, in_channels=32, out_channels=16,
               use_rotary_positional_embeddings=True, use_learned_positional_embeddings=True)
    m = CogVideoXTransformer3DModel(**cfg).init_weights(3)
    sd = m.state_dict()
    assert sd["patch_embed.pos_embedding"].shape == (1, 10 + 2 * 3 * 4, 128)
    assert "patch_embed.pos_embedding" not in dict(m.named_parameters())        # never trained
    assert sd["patch_embed.proj.weight"].shape == (128, 32, 2, 2) and sd["proj_out.weight"].shape == (64, 128)
    with pytest.raises(ValueError):                       # RoPE model called without tables (and vice versa): loud
        m(hidden_states=torch.zeros(1, 2, 32, 6, 8, dtype=torch.bfloat16), encoder_hidden_states=torch.zeros(1, 10, 64),
          timestep=torch.zeros(1, dtype=torch.long))
    root = tmp_path / "CogVideoX-5b-I2V" / "transformer"
    root.mkdir(parents=True)
    (root / "config.json").write_text(json.dumps(cfg))
    table = torch.randn(sd["patch_embed.pos_embedding"].shape).to(torch.bfloat16)
    sd = {k: v.contiguous() for k, v in sd.items()}
    sd["patch_embed.pos_embedding"] = table
    save_file(sd, str(root / "diffusion_pytorch_model.safetensors"))
    m2 = CogVideoXTransformer3DModel.from_pretrained(str(tmp_path / "CogVideoX-5b-I2V"), subfolder="transformer")
    assert torch.equal(m2.patch_embed.pos_embedding, table)
    with pytest.raises(ValueError):
        CogVideoXTransformer3DModel(use_learned_positional_embeddings=True, num_layers=1)


def test_checkpoint_io_reference_conventions(tmp_path):
    """PL-style .ckpt written through the workflow's LoRA-only filter (cogvideo_pl.py:781-787), the reference's strict
    LoRA loader (lvdm/ddpm3d.py:406-432) and auto-resume path selection (utils/train_utils.py:251-288)."""
    from types import SimpleNamespace
    from vt355 import checkpoint as C
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.lora import LoraConfig, get_peft_model
    from vt355.workflow import CogVideoXWorkFlow

    def tiny_peft(seed):
        m = CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(seed)
        m.requires_grad_(False)
        return get_peft_model(m, LoraConfig(r=4, lora_alpha=1.0, target_modules=["to_k", "to_q", "to_v", "to_out.0"]))
    src = tiny_peft(0)
    with torch.no_grad():
        for n, p in src.named_parameters():
            if "lora_B" in n:
                p.copy_(torch.randn(p.shape) * 0.01)
    wf = SimpleNamespace(model=src, global_step=37)
    wf.on_save_checkpoint = lambda ck: CogVideoXWorkFlow.on_save_checkpoint(wf, ck)
    path = C.save_checkpoint(wf, str(tmp_path / "run" / "checkpoints" / "last.ckpt"), epoch=3)
    ck = C.load_checkpoint_file(path)                       # weights_only=True
    assert ck["epoch"] == 3 and ck["global_step"] == 37
    assert len(ck["state_dict"]) == 8 and all(k.startswith("model.base_model.model.") and "lora" in k for k in ck["state_dict"])
    dst = tiny_peft(1)
    assert C.load_lora_from_ckpt(dst, path) == 8
    for (n, a), (_, b) in zip(src.named_parameters(), dst.named_parameters()):
        if "lora" in n:
            assert torch.equal(a, b), n
    # strict both ways
    extra = dict(ck); extra["state_dict"] = dict(ck["state_dict"], **{"model.base_model.model.bogus.lora_A.default.weight": torch.zeros(4, 4)})
    torch.save(extra, tmp_path / "extra.ckpt")
    with pytest.raises(RuntimeError, match="was not copied"):
        C.load_lora_from_ckpt(tiny_peft(2), str(tmp_path / "extra.ckpt"))
    fewer = dict(ck); fewer["state_dict"] = {k: v for i, (k, v) in enumerate(ck["state_dict"].items()) if i}
    torch.save(fewer, tmp_path / "fewer.ckpt")
    with pytest.raises(RuntimeError, match="not found"):
        C.load_lora_from_ckpt(tiny_peft(2), str(tmp_path / "fewer.ckpt"))
    # auto-resume: last.ckpt when readable, else the newest other checkpoint, None without a checkpoints dir
    assert C.get_autoresume_path(str(tmp_path / "run")) == path
    assert C.get_autoresume_path(str(tmp_path / "nothing")) is None
    C.save_checkpoint(wf, str(tmp_path / "run" / "checkpoints" / "epoch=0002.ckpt"), epoch=2)
    (tmp_path / "run" / "checkpoints" / "last.ckpt").write_bytes(b"truncated")
    assert C.get_autoresume_path(str(tmp_path / "run")).endswith("epoch=0002.ckpt")
    # full-state round trip (full fine-tune recipes keep every weight: no 'lora' key -> nothing filtered)
    base = CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(4)
    wf2 = SimpleNamespace(model=base, global_step=5)
    wf2.on_save_checkpoint = lambda ck: CogVideoXWorkFlow.on_save_checkpoint(wf2, ck)
    p2 = C.save_checkpoint(wf2, str(tmp_path / "full.ckpt"))
    other = CogVideoXTransformer3DModel(num_layers=1, num_attention_heads=2, time_embed_dim=64, text_embed_dim=64).init_weights(9)
    wf3 = SimpleNamespace(model=other, global_step=0)
    C.load_full_checkpoint(wf3, p2)
    assert wf3.global_step == 5 and all(torch.equal(a, b) for a, b in zip(base.state_dict().values(), other.state_dict().values()))


def test_encoder_prefetcher_sequencing():
    """vt355.prefetch: batches come out in order, each encoded exactly once, `depth` batches ahead of the consumer."""
    from vt355.prefetch import EncoderPrefetcher
    log = []

    def encode(raw):
        log.append(("enc", raw["i"]))
        return {"latents": torch.full((2, 3), float(raw["i"])), "prompt_embeds": [torch.ones(1) * raw["i"]]}
    got = []
    for b in EncoderPrefetcher(({"i": i} for i in range(5)), encode, device="cpu", depth=2):
        log.append(("use", int(b["latents"][0, 0])))
        got.append(int(b["prompt_embeds"][0]))
    assert got == [0, 1, 2, 3, 4]
    assert log[:4] == [("enc", 0), ("enc", 1), ("enc", 2), ("use", 0)]          # two batches ahead
    assert [x for x in log if x[0] == "enc"] == [("enc", i) for i in range(5)]
    with pytest.raises(ValueError):
        EncoderPrefetcher([], encode, depth=0)


def test_t5_encoder_host_side(tmp_path):
    """HF key names / shapes of the T5 encoder, the sharded safetensors loader, the reflection remap of the reference's
    cond_stage_config, the bucket table against the oracle -- and no CPU path."""
    import json
    import sys
    from safetensors.torch import save_file
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import t5_oracle as T
    from vt355.config import get_obj_from_str
    from vt355.t5 import FrozenT5Embedder, T5EncoderModel, relative_position_bucket
    cfg = T.tiny_config()
    m = T5EncoderModel(**vars(cfg)).init_weights(3)
    want = T.init_params(cfg, 0)
    got = m.state_dict()
    assert set(got) == set(want)
    for k, v in want.items():
        assert tuple(got[k].shape) == tuple(v.shape), k
    rel = torch.arange(-300, 300)
    assert torch.equal(relative_position_bucket(rel, 32, 128), T.relative_position_bucket(rel, 32, 128))
    # sharded HF layout round trip (+ the tied embed_tokens alias the checkpoints carry)
    root = tmp_path / "text_encoder"
    root.mkdir()
    (root / "config.json").write_text(json.dumps(dict(vars(cfg), feed_forward_proj="gated-gelu", model_type="t5", is_encoder_decoder=False)))
    keys = sorted(got)
    half = len(keys) // 2
    shards = {"model-00001-of-00002.safetensors": keys[:half], "model-00002-of-00002.safetensors": keys[half:]}
    wm = {}
    for fn, ks in shards.items():
        sd = {k: got[k].contiguous() for k in ks}
        if "shared.weight" in sd:
            sd["encoder.embed_tokens.weight"] = sd["shared.weight"].clone()
            wm["encoder.embed_tokens.weight"] = fn
        save_file(sd, str(root / fn))
        wm.update({k: fn for k in ks})
    (root / "model.safetensors.index.json").write_text(json.dumps({"weight_map": wm}))
    m2 = T5EncoderModel.from_pretrained(str(tmp_path), subfolder="text_encoder")
    for k, v in got.items():
        assert torch.equal(m2.state_dict()[k], v), k
    assert get_obj_from_str("videotuna.models.lvdm.modules.encoders.condition.FrozenT5Embedder") is FrozenT5Embedder
    emb = FrozenT5Embedder(tokenizer=lambda text, **kw: {"input_ids": torch.zeros(len(text), kw["max_length"], dtype=torch.long)},
                           transformer=m, device="cpu", max_length=12)
    assert not any(p.requires_grad for p in emb.parameters())
    with pytest.raises((ValueError, RuntimeError)):          # host tensors: the kernels have no CPU path
        emb(["a prompt"])
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 4, dtype=torch.long), attention_mask=torch.ones(1, 4))


def test_vae_encoder_host_side():
    """module tree / parameter names of the VAE encoder = the reference's in-tree twin (and the oracle's init_params), shapes, and
    the reference's call surface .encode(x).latent_dist / .config.scaling_factor; no CPU path"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import vae_oracle as V
    from vt355.vae import CogVideoXVaeEncoder, DiagonalGaussianDistribution
    cfg = V.tiny_config(ch=64)
    m = CogVideoXVaeEncoder(ch=cfg.ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks, z_channels=cfg.z_channels,
                            temporal_compress_times=cfg.temporal_compress_times)
    want = V.init_params(cfg, 0)
    got = m.state_dict()
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:6]
    for k, v in want.items():
        assert tuple(got[k].shape) == tuple(v.shape), k
    m.load_state_dict(want)
    assert abs(m.config.scaling_factor - 1.15258426) < 1e-9
    # a whole-autoencoder checkpoint of the twin: encoder sub-tree taken, the rest ignored; safetensors file round trip
    import tempfile
    from safetensors.torch import save_file
    full_ckpt = {"first_stage_model.encoder." + k: v for k, v in want.items()}
    full_ckpt["first_stage_model.decoder.conv_in.conv.weight"] = torch.zeros(3)
    m.load_state_dict(full_ckpt)
    with tempfile.TemporaryDirectory() as d:
        save_file({"encoder." + k: v.contiguous() for k, v in want.items()}, os.path.join(d, "model.safetensors"))
        m3 = CogVideoXVaeEncoder.from_pretrained(d, ch=cfg.ch, ch_mult=cfg.ch_mult, num_res_blocks=cfg.num_res_blocks,
                                                 z_channels=cfg.z_channels, temporal_compress_times=cfg.temporal_compress_times)
    for k, v in want.items():
        assert torch.equal(m3.state_dict()[k], v.to(torch.bfloat16)), k
    d = DiagonalGaussianDistribution(torch.zeros(1, 8, 2, 3, 3))
    assert tuple(d.sample().shape) == (1, 4, 2, 3, 3) and torch.equal(d.mode(), torch.zeros(1, 4, 2, 3, 3))
    full = CogVideoXVaeEncoder()
    assert sum(p.numel() for p in full.parameters()) > 50e6          # CogVideoX encoder: ch 128, (1,2,2,4), 3 blocks per level
    with pytest.raises((ValueError, RuntimeError)):
        m(torch.zeros(1, 3, 5, 8, 8))


REF_CFG = "/root/reference/configs/004_cogvideox"


@pytest.mark.skipif(not os.path.isdir(REF_CFG), reason="the reference tree only exists in the build container")
@pytest.mark.parametrize("yaml_name", ["cogvideo2b.yaml", "cogvideo5b.yaml", "cogvideo5b-i2v.yaml", "cogvideo5b-t2v-fullft.yaml",
                                       "cogvideo5b-i2v-fullft.yaml"])
def test_reference_yaml_files_load_unchanged(tmp_path, monkeypatch, yaml_name):
    """Every configs/004_cogvideox/*.yaml of the reference, read from the reference tree AS IS: config.load_yaml (incl. the
    ${YOUR_DATA_CSV_PATH} placeholders) -> instantiate_from_config(model node) (videotuna/utils/common_utils.py:90-109 semantics,
    targets remapped) against a fake local `checkpoints/` directory of tiny dimensions -> configure_optimizers() -> the LoRA-only
    state_dict filter (cogvideo_pl.py:90-149, 774-787).  `data:` / `lightning:` nodes are read but not built (control plane)."""
    import json
    from safetensors.torch import save_file
    from vt355.config import instantiate_from_config, load_yaml
    from vt355.dit import CogVideoXTransformer3DModel
    from vt355.vae import CogVideoXVaeEncoder
    from vt355.workflow import CogVideoXI2V, CogVideoXWorkFlow
    cfg = load_yaml(os.path.join(REF_CFG, yaml_name), env={"YOUR_DATA_CSV_PATH": "/data/my.csv"})
    assert set(cfg) >= {"model", "data", "lightning"}
    if "5b" in yaml_name:
        assert cfg["data"]["params"]["train"]["params"]["csv_path"] == "/data/my.csv"
    node = cfg["model"]
    i2v, fullft = "i2v" in yaml_name, "fullft" in yaml_name
    root = node["params"]["denoiser_config"]["params"]["pretrained_model_name_or_path"]
    assert root.startswith("checkpoints/cogvideo/CogVideoX-")
    # ---- fake local checkpoint, HF directory layout, tiny dimensions ----
    ck = tmp_path / root
    tcfg = dict(num_attention_heads=1, attention_head_dim=64, num_layers=2, time_embed_dim=64, text_embed_dim=64,
                in_channels=32 if i2v else 16, out_channels=16, sample_width=8, sample_height=4, sample_frames=5,
                max_text_seq_length=4, use_rotary_positional_embeddings="5b" in yaml_name,
                use_learned_positional_embeddings=i2v)
    (ck / "transformer").mkdir(parents=True); (ck / "scheduler").mkdir(); (ck / "vae").mkdir()
    tiny = CogVideoXTransformer3DModel(**tcfg).init_weights(3)
    (ck / "transformer" / "config.json").write_text(json.dumps(tcfg))
    save_file({k: v.contiguous() for k, v in tiny.state_dict().items()}, str(ck / "transformer" / "diffusion_pytorch_model.safetensors"))
    (ck / "scheduler" / "scheduler_config.json").write_text(json.dumps(
        {"_class_name": "CogVideoXDPMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012,
         "snr_shift_scale": 1.0 if "5b" in yaml_name else 3.0}))
    vcfg = dict(ch=64, ch_mult=[1, 2], num_res_blocks=1, z_channels=16, temporal_compress_times=2, scaling_factor=0.7)
    venc = CogVideoXVaeEncoder(**vcfg).init_weights(1)
    (ck / "vae" / "config.json").write_text(json.dumps(vcfg))
    save_file({k: v.contiguous() for k, v in venc.state_dict().items()}, str(ck / "vae" / "diffusion_pytorch_model.safetensors"))
    monkeypatch.chdir(tmp_path)              # the YAMLs name the checkpoints relative to the working directory, as the reference runs
    wf = instantiate_from_config(node)
    assert type(wf) is (CogVideoXI2V if i2v else CogVideoXWorkFlow)
    assert wf.vae.config.scaling_factor == 0.7 and callable(wf.first_stage)      # first_stage_config honoured (local weights)
    assert wf.cond_stage is None                                                   # "DeepFloyd/t5-v1_1-xxl" is a hub name: not fetchable
    assert wf.scheduler.config.num_train_timesteps == 1000
    assert wf.model.config.num_layers == 2 and wf.model.gradient_checkpointing
    assert all(p.dtype == torch.bfloat16 for n, p in wf.model.named_parameters() if "lora" not in n)
    wf.learning_rate = node["base_learning_rate"]           # scripts/train.py:180-185 sets it on the instance
    sd = wf.state_dict()
    if fullft:
        assert not any("lora" in k for k in sd)
        assert all(p.requires_grad for p in wf.model.parameters())
        kept = wf.on_save_checkpoint({"state_dict": dict(sd)})["state_dict"]
        assert set(kept) == set(sd)                         # no adapter -> the full state is saved (cogvideo_pl.py:781-787)
    else:
        lora = {k for k in sd if "lora" in k}
        assert len(lora) == 2 * 4 * 2 and all(".lora_A.default.weight" in k or ".lora_B.default.weight" in k for k in lora)
        opt = wf.configure_optimizers()
        assert sum(p.numel() for p in opt.params) == 2 * 4 * 2 * 4 * 64 and opt.defaults["lr"] == node["base_learning_rate"]
        kept = wf.on_save_checkpoint({"state_dict": dict(sd)})["state_dict"]
        assert set(kept) == lora                            # LoRA-only filter


def test_workflow_survives_a_diffusers_keyed_vae_directory(tmp_path, monkeypatch):
    """The reference's standard HF download holds the VAE under diffusers' key names (encoder.down_blocks.N.resnets.M...), which this
    encoder does not map.  Such a directory must not break the constructor (pre-encoded batches train without the VAE): the stage stays
    unset with a warning, and only a raw {'video', 'caption'} batch raises."""
    import json
    from safetensors.torch import save_file
    from vt355.config import instantiate_from_config
    from vt355.dit import CogVideoXTransformer3DModel
    root = "checkpoints/cogvideo/CogVideoX-2b"
    ck = tmp_path / root
    tcfg = dict(num_attention_heads=1, attention_head_dim=64, num_layers=1, time_embed_dim=64, text_embed_dim=64, in_channels=16,
                out_channels=16, sample_width=8, sample_height=4, sample_frames=5, max_text_seq_length=4)
    (ck / "transformer").mkdir(parents=True); (ck / "scheduler").mkdir(); (ck / "vae").mkdir()
    tiny = CogVideoXTransformer3DModel(**tcfg).init_weights(3)
    (ck / "transformer" / "config.json").write_text(json.dumps(tcfg))
    save_file({k: v.contiguous() for k, v in tiny.state_dict().items()}, str(ck / "transformer" / "diffusion_pytorch_model.safetensors"))
    (ck / "scheduler" / "scheduler_config.json").write_text(json.dumps(
        {"_class_name": "CogVideoXDPMScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012, "snr_shift_scale": 3.0}))
    (ck / "vae" / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKLCogVideoX", "scaling_factor": 1.15258426}))
    save_file({"encoder.conv_in.conv.weight": torch.zeros(128, 3, 3, 3, 3),
               "encoder.down_blocks.0.resnets.0.norm1.norm_layer.weight": torch.zeros(128),
               "decoder.conv_in.conv.weight": torch.zeros(4)}, str(ck / "vae" / "diffusion_pytorch_model.safetensors"))
    monkeypatch.chdir(tmp_path)
    node = {"target": "videotuna.models.cogvideo_hf.cogvideo_pl.CogVideoXWorkFlow", "params": {
        "first_stage_config": {"target": "diffusers.AutoencoderKLCogVideoX",
                               "params": {"pretrained_model_name_or_path": root, "subfolder": "vae"}},
        "cond_stage_config": {"target": "videotuna.lvdm.modules.encoders.condition.FrozenT5Embedder",
                              "params": {"version": "DeepFloyd/t5-v1_1-xxl", "device": "cuda", "max_length": 226, "freeze": True}},
        "denoiser_config": {"target": "diffusers.CogVideoXTransformer3DModel",
                            "params": {"pretrained_model_name_or_path": root, "subfolder": "transformer"}},
        "scheduler_config": {"target": "diffusers.CogVideoXDPMScheduler",
                             "params": {"pretrained_model_name_or_path": root, "subfolder": "scheduler"}}}}
    with pytest.warns(UserWarning, match="could not be loaded"):
        wf = instantiate_from_config(node)
    assert wf.first_stage is None and not hasattr(wf, "vae")
    with pytest.raises(RuntimeError, match="no frozen VAE"):
        wf.get_batch_input({"video": torch.zeros(1, 3, 5, 8, 8), "caption": ["x"]})
    b = wf.get_batch_input({"latents": torch.zeros(1, 16, 2, 4, 8), "prompt_embeds": torch.zeros(1, 4, 64)})
    assert set(b) == {"videos", "prompt_embeds"}


def _tiny_vc2_flow(**kw):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import unet_oracle as U
    from vt355.lvdm import LVDMFlow
    cfg = U.tiny_config()
    unet = dict(target="videotuna.models.lvdm.modules.networks.openaimodel3d.UNetModel", params=dict(
        in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=cfg.model_channels,
        attention_resolutions=list(cfg.attention_resolutions), num_res_blocks=cfg.num_res_blocks, channel_mult=list(cfg.channel_mult),
        num_head_channels=64, transformer_depth=1, context_dim=cfg.context_dim, use_linear=True, use_checkpoint=True, temporal_conv=True,
        temporal_attention=True, temporal_selfatt_only=True, use_relative_position=False, use_causal_attention=False,
        temporal_length=cfg.temporal_length, addition_attention=True, fps_cond=True))
    return U, cfg, LVDMFlow(unet_config=unet, **kw)


def test_vc2_lora_injection_names_and_checkpoint_round_trip(tmp_path):
    """LVDMFlow(lora_args=...) + inject_lora() (ddpm3d.py:100-117, 434-445): adapters on to_q / to_k / to_v of every CrossAttention under
    peft's names, base frozen; the LoRA-only checkpoint filter (callbacks.py:44-46) and load_lora_from_ckpt's two-way strictness
    (ddpm3d.py:406-432) on a file written with the reference's key convention `model.<peft name>`"""
    from vt355.checkpoint import checkpoint_dict, save_checkpoint
    U, cfg, flow = _tiny_vc2_flow(lora_args={"target_modules": ["to_q", "to_k", "to_v"], "lora_rank": 4, "lora_alpha": 1, "lora_dropout": 0.0})
    assert len(flow.lora_args) != 0
    flow.inject_lora()
    flow.inject_lora()                                    # idempotent
    want = {"model.base_model.model.diffusion_model." + k for k in U.init_lora(cfg) if k != U.LORA_SCALING_KEY}
    got = {n for n, p in flow.named_parameters() if "lora" in n}
    assert got == want and len(got) == 180
    assert all(p.requires_grad == ("lora" in n) for n, p in flow.named_parameters())
    B = {n: p for n, p in flow.named_parameters() if ".lora_B." in n}
    assert all(float(p.detach().abs().max()) == 0.0 for p in B.values())              # peft's init: B = 0, A random
    assert all(float(p.detach().abs().max()) > 0.0 for n, p in flow.named_parameters() if ".lora_A." in n)
    ck = checkpoint_dict(flow)
    assert set(ck["state_dict"]) == {"model." + k[len("model."):] for k in want}        # only "lora" keys are written
    with torch.no_grad():
        for p in B.values():
            p.fill_(0.25)
    path = save_checkpoint(flow, str(tmp_path / "lora.ckpt"))
    _, _, flow2 = _tiny_vc2_flow(lora_args={"lora_ckpt": path, "target_modules": ["to_q", "to_k", "to_v"], "lora_rank": 4})
    flow2.inject_lora()                                   # resumes from lora_ckpt
    assert all(float((p.detach() - 0.25).abs().max()) == 0.0 for n, p in flow2.named_parameters() if ".lora_B." in n)
    bad = torch.load(path, weights_only=True)
    bad["state_dict"]["model.extra.lora_A.default.weight"] = torch.zeros(1)
    torch.save(bad, str(tmp_path / "bad.ckpt"))
    with pytest.raises(RuntimeError, match="was not copied"):
        flow2.load_lora_from_ckpt(flow2.model, str(tmp_path / "bad.ckpt"))
    with pytest.raises(NotImplementedError):
        _tiny_vc2_flow(lora_args={"lora_dropout": 0.1})
    _, _, f16 = _tiny_vc2_flow(lora_args={"lora_rank": 16, "lora_alpha": 16})
    f16.inject_lora()                                     # ranks up to 16 (3 x 16 <= 64 extension columns)
    assert f16.unet.lora.r == 16 and f16.unet.lora.scaling == 1.0
    with pytest.raises(ValueError):
        _tiny_vc2_flow(lora_args={"lora_rank": 32})[2].inject_lora()


def test_vc2_random_uncond_rule():
    """classifier-free-guidance dropout of the condition (ddpm3d.py:460-461, 534-535, 710-722): per sample with probability uncond_prob the
    context becomes the empty prompt's embedding (empty_seq) or zeros (zero_embed); off in eval mode and at uncond_prob 0; an empty_seq
    recipe without the empty-prompt embedding fails loudly instead of silently training another objective"""
    import random
    _, cfg, flow = _tiny_vc2_flow()
    assert flow.uncond_prob == 0.2 and flow.uncond_type == "empty_seq"                  # the reference's defaults
    ctx = torch.randn(4, 77, cfg.context_dim)
    null = torch.randn(77, cfg.context_dim)
    out = flow.random_uncond(ctx, null, drop=[True, False, False, True])
    assert torch.equal(out[0], null) and torch.equal(out[3], null) and torch.equal(out[1:3], ctx[1:3])
    with pytest.raises(RuntimeError, match="empty prompt"):
        flow.random_uncond(ctx, None, drop=[True, False, False, False])
    assert flow.random_uncond(ctx, None, drop=[False] * 4) is ctx
    flow.null_context = null
    random.seed(7)
    n_drop = sum(int(torch.equal(flow.random_uncond(ctx[:1])[0], null)) for _ in range(2000))
    assert abs(n_drop / 2000 - 0.2) < 0.03
    random.seed(7)
    want = [random.random() < 0.2 for _ in range(4)]
    random.seed(7)
    o2 = flow.random_uncond(ctx)
    assert [bool(torch.equal(o2[i], null)) for i in range(4)] == want                   # one python random.random() per sample, in order
    flow.eval()
    assert flow.random_uncond(ctx, drop=[True] * 4) is ctx
    _, _, fz = _tiny_vc2_flow(uncond_type="zero_embed", uncond_prob=1.0)
    assert float(fz.random_uncond(ctx).abs().max()) == 0.0
    _, _, f0 = _tiny_vc2_flow(uncond_prob=0.0)
    assert f0.random_uncond(ctx) is ctx


@pytest.mark.skipif(not os.path.isdir("/root/reference/configs"), reason="the reference tree only exists in the build container")
def test_videocrafter2_and_opensora_yaml_files_load_unchanged():
    """configs/001_videocrafter2/vc2_t2v_320x512.yaml (flow style) and configs/003_opensora/opensorav10_256x256.yaml (model style) from the
    reference tree AS THEY ARE: load_yaml -> instantiate_from_config through the target remap -> the denoisers at their real sizes with the
    reference's parameter counts (UNet 1 413 M, STDiT-XL/2 759.6 M).  The frozen first / cond stage
    nodes (VAE, CLIP / T5) are accepted and not built (outside the hot path)."""
    from vt355.config import instantiate_from_config, load_yaml
    from vt355.lvdm import LVDMFlow
    from vt355.stdit import OpenSoraFlow
    vc2 = instantiate_from_config(load_yaml("/root/reference/configs/001_videocrafter2/vc2_t2v_320x512.yaml")["flow"])
    assert isinstance(vc2, LVDMFlow) and vc2.use_scale and abs(vc2.scale_arr[999].item() - 0.7) < 1e-6 and vc2.parameterization == "eps"
    n = sum(p.numel() for p in vc2.model.parameters())
    assert abs(n - 1413.3e6) < 0.5e6, n
    assert vc2.scheduler.num_timesteps == 1000 and abs(vc2.scheduler.alphas_cumprod[0].item() - 0.99915) < 1e-5
    # the LoRA recipe (model style, lora_args: to_q / to_k / to_v, rank 4, alpha 1): scripts/train.py:168-169 then calls inject_lora()
    lo = instantiate_from_config(load_yaml("/root/reference/configs/001_videocrafter2/vc2_t2v_lora.yaml")["model"])
    assert isinstance(lo, LVDMFlow) and len(lo.lora_args) != 0 and lo.lora_rank == 4 and lo.lora_alpha == 1.0
    assert sorted(lo.target_modules) == ["to_k", "to_q", "to_v"] and lo.use_scale and lo.uncond_type == "empty_seq" and lo.uncond_prob == 0.2
    lo.inject_lora()
    names = [n for n, p_ in lo.named_parameters() if p_.requires_grad]
    assert names and all(n.startswith("model.base_model.model.diffusion_model.") and (".lora_A.default.weight" in n or ".lora_B.default.weight" in n)
                         for n in names)
    assert len(names) == 2 * 3 * 2 * 33           # (16 SpatialTransformer + 16 TemporalTransformer + init_attn) x (attn1, attn2) x (q, k, v) x (A, B)
    assert sum(p_.numel() for p_ in lo.parameters() if p_.requires_grad) == 1253888
    osr = instantiate_from_config(load_yaml("/root/reference/configs/003_opensora/opensorav10_256x256.yaml")["model"])
    assert isinstance(osr, OpenSoraFlow) and osr.use_scale
    m = osr.model
    assert (m.depth, m.hidden_size, m.num_heads, m.num_temporal, m.num_spatial) == (28, 1152, 16, 16, 256)
    n = sum(p.numel() for p in m.parameters())
    assert abs(n - 759.6e6) < 0.5e6, n
    assert callable(osr.configure_optimizers) and osr.scheduler.num_timesteps == 1000


def test_encoding_cache_hits_and_resampling():
    """vt355.prefetch.EncodingCache: prompt embeddings by caption (the encoder runs once per distinct caption), latent moments by index
    (the posterior runs once per index, every hit re-draws the sample), byte bound evicts the oldest entries"""
    from types import SimpleNamespace
    from vt355.prefetch import EncodingCache
    calls = {"text": [], "vae": 0}

    def enc(caps):
        calls["text"].append(list(caps))
        return torch.stack([torch.full((4, 8), float(len(c))) for c in caps])

    def post(v):
        calls["vae"] += 1
        return SimpleNamespace(mean=v[:, :2] * 0 + 3.0, std=v[:, :2] * 0 + 0.5)

    ec = EncodingCache()
    e1 = ec.prompt_embeds(["a", "bb", "a"], enc)
    e2 = ec.prompt_embeds(["bb", "ccc"], enc)
    assert calls["text"] == [["a", "bb"], ["ccc"]] and e1.shape == (3, 4, 8) and torch.equal(e1[0], e1[2]) and e2[1, 0, 0] == 3
    vids = [torch.zeros(3, 5, 4, 4), torch.zeros(3, 5, 4, 4)]
    g = torch.Generator().manual_seed(0)
    l1 = ec.latents([7, 9], vids, post, 0.7, generator=g)
    l2 = ec.latents(torch.tensor([9, 7]), vids, post, 0.7, generator=g)
    assert calls["vae"] == 2 and l1.shape == (2, 2, 5, 4, 4) and not torch.equal(l1[0], l2[1])       # same moments, fresh noise
    assert abs(l2.mean().item() - 3.0 * 0.7) < 0.1 and ec.hits == {"text": 2, "latent": 2}
    small = EncodingCache(max_bytes=4 * 8 * 4 * 2)
    small.prompt_embeds(["x", "yy", "zzz"], enc)
    assert list(small.text) == ["yy", "zzz"]


def test_hunyuan_rope_tables_and_remap():
    """vt355.hunyuan.rope_tables vs the reference's get_nd_rotary_pos_embed (tests/golden/hunyuan_rope.npz: rope_dim_list [16, 56, 56], sizes
    [3, 4, 6], theta 256); the in-tree denoiser / workflow targets resolve through the remap table"""
    import numpy as np
    from vt355.config import get_obj_from_str
    from vt355.hunyuan import HYVideoDiffusionTransformer, HunyuanVideoFlow, rope_tables
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hunyuan_rope.npz"))
    cos, sin = rope_tables((3, 4, 6))
    assert np.allclose(cos.numpy(), g["cos"], atol=1e-6) and np.allclose(sin.numpy(), g["sin"], atol=1e-6)
    assert get_obj_from_str("videotuna.models.hunyuan.hyvideo_t2v.modules.models.HYVideoDiffusionTransformer") is HYVideoDiffusionTransformer
    assert get_obj_from_str("videotuna.models.hunyuan.hyvideo_t2v.hunyuanvideo.HunyuanVideoWorkFlow") is HunyuanVideoFlow
    m = HYVideoDiffusionTransformer(in_channels=4, hidden_size=256, heads_num=2, mm_double_blocks_depth=1, mm_single_blocks_depth=1,
                                    text_states_dim=64, text_states_dim_2=32, lora_rank=4)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 4, 1, 4, 4), torch.zeros(1))                       # no CPU fallback


def test_flat_layouts_the_batched_paths_rely_on(monkeypatch):
    """Host side of the batched small-tensor paths: (1) STDiT's blocks sit at a constant stride in the flat parameter buffer, so one
    as_strided view addresses the same parameter of all blocks (stdit.block_stride; VT355_STDIT_BATCH=0 switches the batching off);
    (2) the HunyuanVideo adapters' flat buffer is [A_0 | B_0 | A_1 | B_1 ...] with one [r, D] + [D, r] pair per adapter in site order,
    which is what the stacked refresh / gradient scatter index"""
    import stdit_oracle as SO
    from vt355.stdit import STDiT, block_stride, _PAD_SITES
    cfg = SO.tiny_config()
    m = STDiT(input_size=cfg.input_size, in_channels=cfg.in_channels, patch_size=cfg.patch_size, hidden_size=cfg.hidden_size, depth=cfg.depth,
              num_heads=cfg.num_heads, mlp_ratio=cfg.mlp_ratio, class_dropout_prob=0.0, caption_channels=cfg.caption_channels,
              model_max_length=cfg.model_max_length, space_scale=cfg.space_scale, time_scale=cfg.time_scale)
    monkeypatch.delenv("VT355_STDIT_BATCH", raising=False)
    names = [suf + ".weight" for suf, _, _ in _PAD_SITES] + [suf + ".bias" for suf, kind, _ in _PAD_SITES if kind == "rows"] + ["scale_shift_table"]
    for suf in names:
        lay = block_stride(m, suf)
        assert lay is not None, suf
        off0, st = lay
        for i in range(cfg.depth):
            assert m.offsets[f"blocks.{i}.{suf}"] == off0 + i * st
        v = m.flat_bf16.as_strided((cfg.depth, 4), (st, 1), off0)                      # the first elements of every block's copy
        for i in range(cfg.depth):
            assert v[i].data_ptr() == m._plist[f"blocks.{i}.{suf}"].data_ptr()
    assert block_stride(m, "no.such.parameter") is None
    monkeypatch.setenv("VT355_STDIT_BATCH", "0")
    assert block_stride(m, "scale_shift_table") is None

    from vt355.hunyuan import HunyuanBlocks
    D, r = 256, 4
    hb = HunyuanBlocks(hidden_size=D, heads_num=2, mm_double_blocks_depth=2, mm_single_blocks_depth=3, lora_rank=r, lora_alpha=2.0)
    L = hb.lora
    s = 0
    for mod, tags in L.sites.items():
        for t in tags:
            dot = "." + t if t else ""
            assert L.offsets[f"{mod}.lora_A{dot}.weight"] == 2 * s * r * D and L.shapes[f"{mod}.lora_A{dot}.weight"] == (r, D)
            assert L.offsets[f"{mod}.lora_B{dot}.weight"] == (2 * s + 1) * r * D and L.shapes[f"{mod}.lora_B{dot}.weight"] == (D, r)
            s += 1
    assert s == 2 * 4 + 3 * 3 and L.numel == 2 * s * r * D
