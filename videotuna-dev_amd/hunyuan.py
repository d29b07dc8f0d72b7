"""HunyuanVideo transformer trunk on the vt355 kernels (BASELINE configs[4]): the double-stream and
single-stream blocks of videotuna/models/hunyuan/hyvideo_t2v/modules/models.py (MMDoubleStreamBlock :21-252, MMSingleStreamBlock :255-393)
with the parameter names of ``HYVideoDiffusionTransformer.double_blocks / single_blocks``, forward and backward (full fine-tune tape of
vt355.unet), plus the flow-matching loss of ``HunyuanVideoWorkFlow.training_step`` (hyvideo_t2v/hunyuanvideo.py:923-971).

What runs where: SiLU -> Linear modulation (small GEMM, fp32 out); LayerNorm(no affine) + modulate in vt_ln_modulate; fused qkv GEMM;
per-head RMS q/k norm + rotary embedding of the image tokens + the [image; text] concatenation in ONE pass (vt_qk_rmsnorm_rope128);
joint attention with per-sample valid lengths through vt_attn128_fwd / _bwd (the long-sequence head_dim-128 kernels); projections / MLPs with GELU-tanh and gated
residuals in the GEMM epilogues; the single block's ``linear1`` split into its qkv and MLP row ranges (the GELU lives in the second
GEMM's epilogue, both write into one [attn | gelu(mlp)] buffer that ``linear2`` reads).
``fp8=True`` (or ``"weights"``) is the reference's fp8 mode (fp8_optimization.py:55-101): EVERY Linear of the double / single blocks -- qkv,
proj, the MLPs, linear1 / linear2, the modulation Linears -- holds its weight as E4M3 with a per-tensor scale (max|W| / 448) and computes
``F.linear(x, dequant(W))`` in bf16; here the de-quantised bf16 copies are the GEMM operands (forward and dX), built once per weight version.
``fp8="matmul"`` additionally runs the qkv projections' forward on the fp8 matrix cores (vt_gemm_fp8, activations quantised per tensor on
the fly -- beyond the reference, which never quantises activations); gradients stay bf16.
``fp8="mfma"`` runs the FORWARD product of every double / single block Linear (qkv, proj, fc1, fc2, both row ranges of linear1, linear2;
not the modulation Linears) on the MX-scaled fp8 matrix cores (vt_gemm_mxfp8): E4M3 weights with their per-tensor scale as above, E4M3
activations with a per-site DELAYED scale (max of the last ``fp8_amax_history`` recorded amaxes / 448, fixed for a forward, updated by one
vt_fp8_scale_update launch at its start).  The producer of each quantised input writes the fp8 copy next to its bf16 output (LayerNorm +
modulate, the fc1 / linear1 GELU epilogue, the attention-output split); the first forward (and the first after load_state_dict or a change
of ``fp8``) has no history and scales just in time.  LoRA sites keep their K-extension columns in bf16 (the GEMM's bf16 tail).  The
backward is that of ``"weights"`` mode: bf16, from the saved bf16 activations and the de-quantised weights.
``fp8="mfma", fp8_dgrad=True`` (or ``"e5m2"`` / ``"e4m3"``, the format the gradients are quantised to) additionally runs every
INPUT-GRADIENT product dX = g W of those Linears on the same matrix cores (vt_gemm_mxfp8_dx): the quantised output gradient against the
byte-transposed E4M3 weight, one delayed-scaling site per gradient tensor that feeds such a product (per double block and stream d(qkv),
gated d(proj out), gated d(fc2 out), d(u); per single block gated d(linear2 out), d(qkv), d(u)), scales updated by one launch at the
start of each backward.  The gated gradients are quantised by the gate multiply (vt_gate_mul_fp8), d(u) by the dGELU epilogue of the
product that makes it, d(qkv) by one cast pass.  Parameter gradients keep reading the bf16 gradients; the forward is untouched (beyond the
reference, which never quantises gradients).
LoRA (``lora_rank``, ``lora_target_modules``): rank-r adapters on the image stream's attention projections (the shipped recipe's targets,
the default) and, by name, on its feed-forward Linears -- fc1, fc2, the MLP rows of linear1, linear2 (_HYLora); every adapted Linear stays
ONE GEMM over K-extended operands, forward and input gradient (DESIGN 3 "LoRA as a K-extension").
``lora_dropout`` = p > 0: in training mode every adapter reads its Linear's input under its own Philox keep mask (peft's nn.Dropout in front of
lora_A), recomputed inside the wide rank-side kernels and keyed by the row of the unsharded run (DESIGN 4 "mask convention"); the input
gradient is then the base product plus an in-place masked correction.

NOT built (recorded in DESIGN.md): the embedders / token refiner / final layer of HYVideoDiffusionTransformer, the diffusers
``HunyuanVideoTransformer3DModel`` key map and LoRA wrappers of the shipped recipe, (the head_dim-128 attention backward is atomics-only: no dQ hand-off chains yet).  Padding text rows attend to the valid keys here
(the reference gives them their own segment, attenion.py:34-57); they are never read by valid rows or by the loss.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.distributed

from . import ops
from .engine import lora_dropout_seed
from .lora import extension_layout
from .ops import BF16, EPI_BIAS_GELU, EPI_DGELU, EPI_GATED_RES
from .stdit import _STRun
from .unet import F32, FlatParamModule, _Var


def _double_shapes(D, H, ratio, pre):
    hd, M4 = D // H, int(D * ratio)
    sh = {}
    for s in ("img", "txt"):
        sh[f"{pre}{s}_mod.linear.weight"] = (6 * D, D); sh[f"{pre}{s}_mod.linear.bias"] = (6 * D,)
        sh[f"{pre}{s}_attn_qkv.weight"] = (3 * D, D); sh[f"{pre}{s}_attn_qkv.bias"] = (3 * D,)
        sh[f"{pre}{s}_attn_q_norm.weight"] = (hd,); sh[f"{pre}{s}_attn_k_norm.weight"] = (hd,)
        sh[f"{pre}{s}_attn_proj.weight"] = (D, D); sh[f"{pre}{s}_attn_proj.bias"] = (D,)
        sh[f"{pre}{s}_mlp.fc1.weight"] = (M4, D); sh[f"{pre}{s}_mlp.fc1.bias"] = (M4,)
        sh[f"{pre}{s}_mlp.fc2.weight"] = (D, M4); sh[f"{pre}{s}_mlp.fc2.bias"] = (D,)
    return sh


def _single_shapes(D, H, ratio, pre):
    hd, M4 = D // H, int(D * ratio)
    return {pre + "linear1.weight": (3 * D + M4, D), pre + "linear1.bias": (3 * D + M4,), pre + "linear2.weight": (D, D + M4),
            pre + "linear2.bias": (D,), pre + "q_norm.weight": (hd,), pre + "k_norm.weight": (hd,),
            pre + "modulation.linear.weight": (3 * D, D), pre + "modulation.linear.bias": (3 * D,)}


class _XVar(_Var):
    """an activation that lives in the first D columns of an extended buffer (input of a LoRA'd Linear)"""
    __slots__ = ("ext",)

    def __init__(self, d, ext):
        super().__init__(d)
        self.ext = ext


EXT = 64          # K-extension columns of a LoRA'd Linear: x_ext = [x | x A^T (3 r <= 64 columns) | 0], W_ext = [W | scaling * B | 0]
MAX_R = 128       # ranks with 3 r > EXT: the wide layout of vt355.lora.extension_layout on the MFMA rank-side kernels (csrc/lora_wide.hip)


def lora_layout(r: int, wide: bool = False):
    """(rp, ext_qkv, ext_proj, wide) of the K-extension of a HunyuanVideo adapter of rank r.  3 r <= 64: the three adapters of a fused
    projection sit side by side (column stride rp = r) in a fixed 64-column extension.  Above that -- or at any rank when VT355_LORA_WIDE=1
    is set, a test / A-B knob, or with wide=True (lora_dropout > 0: the narrow layout's rank-side work is stock GEMMs with nowhere to
    mask) -- the wide layout: rp = r rounded up to a multiple of 16, adapter j in columns [j rp, j rp + r), the
    extension 3 rp (q | k | v projections) / rp (img_attn_proj) columns rounded up to a multiple of 64, every other column zero."""
    if r <= 0 or r > MAX_R:
        raise ValueError(f"rank {r}: HunyuanVideo LoRA ranks are 1..{MAX_R} (three adapters of {MAX_R} rank columns fill the widest K-extension)")
    if not wide and 3 * r <= EXT and os.environ.get("VT355_LORA_WIDE", "0") in ("", "0"):
        return r, EXT, EXT, False
    return extension_layout(r, wide=True)


ATTN_TARGETS = ("to_q", "to_k", "to_v", "to_out.0")                       # one group: today's sites
FF_TARGETS = ("ff.net.0.proj", "ff.net.2", "proj_mlp", "proj_out")        # chosen one by one


def resolve_lora_targets(target_modules):
    """(attn, ff) for ``lora_target_modules``: attn -- whether the attention group ATTN_TARGETS is adapted, ff -- the members of FF_TARGETS
    that are, in FF_TARGETS order.  None: the attention group alone (the shipped recipe).  The names are the diffusers / peft names of
    configs/007_hunyuanvideo/hunyuanvideo_t2v_diffuser_lora.yaml; they reach the image stream's Linears of the double blocks and the
    single blocks only -- the token refiner's feed-forward and the model-level proj_out, which peft's suffix rule would also match on
    diffusers' class, stay frozen."""
    if target_modules is None:
        return True, ()
    if isinstance(target_modules, str):
        target_modules = [target_modules]
    names = list(target_modules)
    unknown = [t for t in names if t not in ATTN_TARGETS + FF_TARGETS]
    if unknown:
        raise ValueError(f"unsupported HunyuanVideo LoRA target(s) {unknown}: {ATTN_TARGETS + FF_TARGETS} are supported")
    if not names:
        raise ValueError("lora_target_modules is empty: name targets or pass None for the attention projections")
    got = [t for t in ATTN_TARGETS if t in names]
    if got and len(got) != len(ATTN_TARGETS):
        raise ValueError(f"the attention targets {ATTN_TARGETS} are adapted together (the fused q | k | v projections share one K-extension): "
                         f"{got} alone is not supported")
    return bool(got), tuple(t for t in FF_TARGETS if t in names)


class _HYLora(FlatParamModule):
    """rank-r adapters on the image stream's Linears.  The attention group (the modules the shipped recipe targets, configs/007_hunyuanvideo/
    hunyuanvideo_t2v_diffuser_lora.yaml:59-64: r 4, alpha 1, target_modules to_q / to_k / to_v / to_out.0 of diffusers' attention): the
    q / k / v row blocks of ``double_blocks.N.img_attn_qkv`` and of ``single_blocks.N.linear1`` and ``double_blocks.N.img_attn_proj``.
    Parameter names: ``<module>.lora_A.{q,k,v}.weight [r, D]``, ``<module>.lora_B.{q,k,v}.weight [D, r]`` (proj: no q/k/v level).
    The feed-forward targets (``target_modules``, resolve_lora_targets), one adapter each, behind the attention group's parameters:
    ff.net.0.proj -> ``double_blocks.N.img_mlp.fc1`` (A [r, D], B [4D, r]), ff.net.2 -> ``double_blocks.N.img_mlp.fc2`` (A [r, 4D],
    B [D, r]), proj_mlp -> the MLP rows of ``single_blocks.N.linear1`` (tag ``mlp``: A [r, D], B [4D, r]), proj_out ->
    ``single_blocks.N.linear2`` (A [r, 5D], B [D, r]).
    Ranks 1..128; the K-extension layout (narrow up to 3 r = 64, wide above) is lora_layout's and does not show in names or shapes.
    ``dropout`` = p > 0 (peft's lora_dropout): every adapter reads its Linear's input under its own Philox keep mask in training mode
    (DESIGN 4 "mask convention"); the layout is then the wide one at every rank.  ``site_of``: lora_A name -> adapter site, the adapter's
    position among the lora_A entries of ``shapes`` (q, k, v of a fused projection are consecutive sites)."""

    def __init__(self, D: int, n_double: int, n_single: int, r: int, alpha: float, ratio: float = 4.0, target_modules=None,
                 dropout: float = 0.0):
        super().__init__()
        self.p = float(dropout)
        self.rp, self.ext_qkv, self.ext_proj, self.wide = lora_layout(r, wide=self.p > 0)      # fixed at construction (VT355_LORA_WIDE is read here)
        self.r, self.scaling, self.D = r, alpha / r, D
        self.attn, self.ff_targets = resolve_lora_targets(target_modules)
        sh: Dict[str, tuple] = {}
        self.sites: Dict[str, list] = {}            # module name -> adapter tags (the attention group)
        if self.attn:
            for i in range(n_double):
                self.sites[f"double_blocks.{i}.img_attn_qkv"] = ["q", "k", "v"]
                self.sites[f"double_blocks.{i}.img_attn_proj"] = [""]
            for i in range(n_single):
                self.sites[f"single_blocks.{i}.linear1"] = ["q", "k", "v"]
        for mod, tags in self.sites.items():
            for t in tags:
                dot = "." + t if t else ""
                sh[f"{mod}.lora_A{dot}.weight"] = (r, D)
                sh[f"{mod}.lora_B{dot}.weight"] = (D, r)
        # The feed-forward sites: ONE adapter per site, in the extension columns [0, r) -- the narrow and the wide layout differ in the
        # extension's width only (64 / rp rounded up to 64); t = x A^T and dt = g (scaling B) are bf16 GEMMs with N = ext, the rank
        # gradients run on vt_lora_tn_wide, the pack kernels are the wide layout's with the rank padded to rpf.  ff: site key -> (module, tag, in width, out width, first weight row); the key is the module name, for
        # linear1's MLP rows "<module>#mlp" (the module name is the attention group's q | k | v site).
        M4 = int(D * ratio)
        self.rpf, self.ext_ff = (r + 15) // 16 * 16, self.ext_proj
        self.ff: Dict[str, SimpleNamespace] = {}
        want = set(self.ff_targets)
        for i in range(n_double):
            if "ff.net.0.proj" in want:
                self.ff[f"double_blocks.{i}.img_mlp.fc1"] = SimpleNamespace(mod=f"double_blocks.{i}.img_mlp.fc1", tag="", din=D, dout=M4, row0=0)
            if "ff.net.2" in want:
                self.ff[f"double_blocks.{i}.img_mlp.fc2"] = SimpleNamespace(mod=f"double_blocks.{i}.img_mlp.fc2", tag="", din=M4, dout=D, row0=0)
        for i in range(n_single):
            if "proj_mlp" in want:
                self.ff[f"single_blocks.{i}.linear1#mlp"] = SimpleNamespace(mod=f"single_blocks.{i}.linear1", tag="mlp", din=D, dout=M4, row0=3 * D)
            if "proj_out" in want:
                self.ff[f"single_blocks.{i}.linear2"] = SimpleNamespace(mod=f"single_blocks.{i}.linear2", tag="", din=D + M4, dout=D, row0=0)
        for s in self.ff.values():
            dot = "." + s.tag if s.tag else ""
            s.a_name, s.b_name = f"{s.mod}.lora_A{dot}.weight", f"{s.mod}.lora_B{dot}.weight"
            sh[s.a_name] = (r, s.din)
            sh[s.b_name] = (s.dout, r)
        self._setup_flat(sh)
        self.site_of = {n: i for i, n in enumerate(n for n in self.shapes if ".lora_A" in n)}

    def ext_of(self, mod: str) -> int:
        """K-extension columns of the adapted Linear `mod` of the attention group"""
        return self.ext_qkv if len(self.sites[mod]) == 3 else self.ext_proj

    def init_weights(self, seed: int = 0, zero_b: bool = True):
        """peft's default: A random, B zero (the adapter starts as the identity); zero_b=False for tests"""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self._plist.items():
                if ".lora_A" in n:
                    p.copy_((torch.randn(self.shapes[n], generator=g) * self.shapes[n][1] ** -0.5).to(p.device, BF16))
                else:
                    p.copy_((torch.zeros(self.shapes[n]) if zero_b else torch.randn(self.shapes[n], generator=g) * 0.05).to(p.device, BF16))
        self._packed = None
        return self


class HunyuanBlocks(FlatParamModule):
    """double_blocks.{i}.* / single_blocks.{i}.* of HYVideoDiffusionTransformer (models.py:396-...): hidden_size 3072, 24 heads x 128,
    20 + 40 blocks in HunyuanVideo-T2V"""

    def __init__(self, hidden_size: int = 3072, heads_num: int = 24, mlp_width_ratio: float = 4.0, mm_double_blocks_depth: int = 20,
                 mm_single_blocks_depth: int = 40, fp8: bool = False, lora_rank: int = 0, lora_alpha: float = 1.0,
                 shapes_before: Optional[Dict[str, tuple]] = None, shapes_after: Optional[Dict[str, tuple]] = None, fp8_amax_history: int = 16,
                 fp8_dgrad=False, lora_target_modules=None, lora_dropout: float = 0.0):
        super().__init__()
        if hidden_size // heads_num != 128 or hidden_size % 128:
            raise ValueError("HunyuanVideo heads are 128 wide")
        if not (0.0 <= lora_dropout < 1.0):
            raise ValueError(f"lora_dropout={lora_dropout!r}: a probability 0 <= p < 1")
        if lora_dropout > 0 and lora_rank == 0:
            raise ValueError(f"lora_dropout={lora_dropout!r} without adapters: set lora_rank")
        if lora_dropout > 0 and fp8_dgrad:
            raise NotImplementedError(f"lora_dropout={lora_dropout!r} with fp8_dgrad={fp8_dgrad!r}: the dGELU epilogue's fp8 copy of d(u) would lack "
                                      "the masked adapter term, which is added after the product (DESIGN 8: a vt_cast_fp8_fmt pass after the "
                                      "masked add at the two dGELU gradient sites)")
        self.lora_dropout = float(lora_dropout)
        self.lora_dropout_seed = None        # lora_dropout > 0: None = a fresh mask seed per training forward, an int pins it
        self.last_lora_dropout_seed = None   # the seed the latest training forward used
        if fp8_amax_history < 1:
            raise ValueError("fp8_amax_history: at least one recorded amax")
        self.hidden_size, self.heads_num, self.ratio = hidden_size, heads_num, mlp_width_ratio
        self.fp8_amax_history = fp8_amax_history
        self._fp8_dgrad = False
        self.n_double, self.n_single, self.fp8 = mm_double_blocks_depth, mm_single_blocks_depth, fp8
        sh: Dict[str, tuple] = {}
        for i in range(mm_double_blocks_depth):
            sh.update(_double_shapes(hidden_size, heads_num, mlp_width_ratio, f"double_blocks.{i}."))
        for i in range(mm_single_blocks_depth):
            sh.update(_single_shapes(hidden_size, heads_num, mlp_width_ratio, f"single_blocks.{i}."))
        self._setup_flat({**(shapes_before or {}), **sh, **(shapes_after or {})})
        # LoRA mode: the block weights stay frozen (no fp32 master, no gradients, no dW GEMMs); only the adapters train
        # lora_rank 0: no adapters; 1..MAX_R: _HYLora (which refuses anything else)
        # lora_target_modules: None = the attention projections (resolve_lora_targets); names without a rank are still checked
        if lora_rank == 0:
            resolve_lora_targets(lora_target_modules)
        self.lora = _HYLora(hidden_size, mm_double_blocks_depth, mm_single_blocks_depth, lora_rank, lora_alpha, mlp_width_ratio,
                            lora_target_modules, dropout=lora_dropout) if lora_rank != 0 else None
        self.sp_group = None
        self.fp8_dgrad = fp8_dgrad

    @property
    def fp8(self):
        return self._fp8

    @fp8.setter
    def fp8(self, mode):
        if mode not in (False, True, "weights", "matmul", "mfma"):
            raise ValueError(f"fp8={mode!r}: one of False, True / 'weights', 'matmul', 'mfma'")
        if mode == "mfma" and (self.hidden_size % 128 or int(self.hidden_size * self.ratio) % 128):
            raise ValueError(f"fp8='mfma': the MX-fp8 GEMM needs every block Linear's input width (hidden_size {self.hidden_size}, MLP width "
                             f"{int(self.hidden_size * self.ratio)}) to be a multiple of 128")
        if mode != "mfma" and getattr(self, "_fp8_dgrad", False):
            raise ValueError(f"fp8={mode!r}: fp8_dgrad={self._fp8_dgrad!r} needs fp8='mfma' (set fp8_dgrad = False first)")
        self._fp8 = mode
        self.fp8_reset()

    @property
    def fp8_dgrad(self):
        """False, or the format the output gradients are quantised to for the fp8 dX products: True / 'e5m2', 'e4m3'"""
        return self._fp8_dgrad

    @fp8_dgrad.setter
    def fp8_dgrad(self, mode):
        if not any(mode is v for v in (False, True)) and mode not in ("e5m2", "e4m3"):
            raise ValueError(f"fp8_dgrad={mode!r}: one of False, True / 'e5m2', 'e4m3'")
        if mode and self._fp8 != "mfma":
            raise ValueError(f"fp8_dgrad={mode!r}: the fp8 input-gradient products belong to fp8='mfma' (fp8={self._fp8!r})")
        if mode and getattr(self, "lora_dropout", 0.0) > 0:
            raise NotImplementedError(f"fp8_dgrad={mode!r} with lora_dropout={self.lora_dropout!r}: the dGELU epilogue's fp8 copy of d(u) would "
                                      "lack the masked adapter term (DESIGN 8)")
        self._fp8_dgrad = mode
        self._packed = None                 # the transposed operands change: fp8 bytes instead of bf16 copies
        self.fp8_reset()

    @property
    def fp8_grad_format(self):
        """the gradient format: None, 'e5m2' or 'e4m3'"""
        return None if not self._fp8_dgrad else ("e4m3" if self._fp8_dgrad == "e4m3" else "e5m2")

    @property
    def n_fp8_grad_sites(self) -> int:
        """gradient sites of fp8_dgrad: per double block and stream d(qkv), gated d(proj out), gated d(fc2 out), d(u); per single block
        gated d(linear2 out), d(qkv), d(u)"""
        return 8 * self.n_double + 3 * self.n_single

    @property
    def n_fp8_sites(self) -> int:
        """activation sites of fp8='mfma': per double block and stream the qkv / proj / fc1 / fc2 inputs, per single block linear1 / linear2"""
        return 8 * self.n_double + 2 * self.n_single

    def fp8_reset(self):
        """forget the delayed-scaling history: the next fp8='mfma' forward (and fp8_dgrad backward) scales just in time and seeds it"""
        self._fp8_state = None
        self._fp8_grad_state = None

    def fp8_state(self):
        """(amax, history, scale) device tensors of the activation sites, created (unseeded) on first use"""
        st = self._fp8_state
        if st is None or st.amax.device != self.device:
            n, H = self.n_fp8_sites, self.fp8_amax_history
            st = SimpleNamespace(amax=torch.zeros(n, dtype=F32, device=self.device), history=torch.zeros(n, H, dtype=F32, device=self.device),
                                 scale=torch.ones(n, dtype=F32, device=self.device), seeded=False)
            self._fp8_state = st
        return st

    def fp8_grad_state(self):
        """(amax, history, scale) device tensors of the gradient sites (fp8_dgrad), created (unseeded) on first use"""
        st = self._fp8_grad_state
        if st is None or st.amax.device != self.device:
            n, H = self.n_fp8_grad_sites, self.fp8_amax_history
            st = SimpleNamespace(amax=torch.zeros(n, dtype=F32, device=self.device), history=torch.zeros(n, H, dtype=F32, device=self.device),
                                 scale=torch.ones(n, dtype=F32, device=self.device), seeded=False)
            self._fp8_grad_state = st
        return st

    def load_state_dict(self, sd, strict: bool = True, **kw):
        out = super().load_state_dict(sd, strict=strict, **kw)
        self.fp8_reset()
        return out

    def set_sequence_parallel(self, group):
        """Ulysses sequence parallelism over ``group`` (vt355.sp; SURVEY 8(e), the 119 k-token 720p sequence): ``img`` and ``freqs_cis`` passed
        to forward are then THIS RANK'S contiguous 1/P of the image rows, the text rows are replicated, and the result holds the local image
        rows followed by the text rows.  Every row-wise kernel runs on the local rows; the joint attention exchanges rows for heads around
        ``vt_attn128`` (all rows, H/P heads).  Gradients follow sp.py's partial-sum convention: text-row, modulation-vector and parameter
        gradients of a rank are partial, the group SUM is the gradient (so a data-parallel reducer that averages over all ranks, with every
        rank back-propagating the mean loss of its own rows, yields the gradient of the overall mean).  ``None`` switches it off."""
        if group is not None:
            import torch.distributed as dist
            if self.heads_num % dist.get_world_size(group):
                raise ValueError(f"{self.heads_num} heads do not split over {dist.get_world_size(group)} ranks")
        self.sp_group = group
        return self

    def _sp_rows(self, N: int):
        """(first row, row count) of this rank's image tokens: everything without sequence parallelism"""
        if self.sp_group is None:
            return 0, N
        import torch.distributed as dist
        P, r = dist.get_world_size(self.sp_group), dist.get_rank(self.sp_group)
        if N % P:
            raise ValueError(f"{N} image tokens do not split over {P} ranks")
        return r * (N // P), N // P

    def init_weights(self, seed: int = 0):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for n, p in self._plist.items():
                s = self.shapes[n]
                if len(s) == 1:
                    w = torch.randn(s, generator=g) * 0.05 + (1.0 if "norm.weight" in n else 0.0)
                else:
                    w = torch.randn(s, generator=g) * (0.7 / s[1] ** 0.5)
                p.copy_(w.to(p.device, BF16))
        self._packed = None
        if self.lora is not None:
            self.lora.init_weights(seed + 1)
        return self

    def enable_lora_training(self):
        """training state of the adapters only (hand it to FusedAdamW(ts.params, fullft_state=ts)); the block weights stay frozen"""
        if self.lora is None:
            raise RuntimeError("construct HunyuanBlocks(lora_rank=r) first")
        self.requires_grad_(False)
        self.lora.requires_grad_(True)
        return self.lora.enable_training()

    def forward(self, img, txt, vec, txt_valid, freqs_cis=None):
        """img [B, Li, D], txt [B, Lt, D], vec [B, D] bf16; txt_valid int [B] valid text tokens; freqs_cis = (cos, sin) fp32 [Li, 128]
        -> x [B, Li + Lt, D] = [image; text] after every double and single block (models.py: HYVideoDiffusionTransformer.forward trunk)"""
        if not img.is_cuda:
            raise RuntimeError("vt355 HunyuanBlocks runs only on an MI355X device (no CPU fallback)")
        if torch.is_grad_enabled() and (self.train_state is not None or (self.lora is not None and self.lora.train_state is not None)):
            anchor = torch.zeros(1, device=img.device, requires_grad=True)
            return _HYFn.apply(anchor, self, img, txt, vec, txt_valid, freqs_cis)
        return _HYRun(self, save=False).forward(img, txt, vec, txt_valid, freqs_cis)


class _HYFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, model, img, txt, vec, txt_valid, freqs):
        run = _HYRun(model, save=True)
        run.need_dvec = bool(ctx.needs_input_grad[4])
        out = run.forward(img, txt, vec, txt_valid, freqs)
        ctx.run = run
        return out

    @staticmethod
    def backward(ctx, dout):
        run = ctx.run
        ctx.run = None
        dimg, dtxt, dvec = run.backward(dout)
        return None, None, dimg, dtxt, dvec, None, None


_MFMA_LINEARS = ("_attn_qkv.weight", "_attn_proj.weight", "_mlp.fc1.weight", "_mlp.fc2.weight", "linear1.weight", "linear2.weight")


def _packed_hy(model: HunyuanBlocks) -> SimpleNamespace:
    ver = -1 if model.train_state is None else model.train_state.version
    if model._packed is not None and model._packed_version == ver:
        return model._packed
    P = SimpleNamespace(wt={}, w={}, b={}, q={}, qt={})
    fb = model.flat_bf16
    train = model.train_state is not None or (model.lora is not None and model.lora.train_state is not None)
    dgrad = model.fp8 == "mfma" and bool(model.fp8_dgrad)
    with torch.no_grad():
        for n, shp in model.shapes.items():
            if n.endswith(".weight") and len(shp) == 2:
                w = model.flat(fb, n)
                # an adapted Linear's transposed operand is the extended one (_packed_lora / _pack_ff)
                lora_site = model.lora is not None and (n[:-7] in model.lora.sites or n[:-7] in model.lora.ff)
                if model.fp8:                                       # E4M3 copy + per-tensor scale (fp8_optimization.py:55-64) ...
                    wq, sw = ops.quantize_fp8(w)
                    w = (wq.to(torch.float32) * sw).to(BF16)        # ... and what the reference multiplies with: dequant(W) (:50-53, 72-78)
                    P.w[n] = w
                    if (model.fp8 == "matmul" and n.endswith("_attn_qkv.weight")) or (model.fp8 == "mfma" and n.endswith(_MFMA_LINEARS)):
                        P.q[n] = (wq, sw)               # mfma: linear1's two row ranges share the tensor's one scale
                        if dgrad and train:                                 # fp8 dX: the byte-transposed E4M3 weight, same scale
                            P.qt[n] = wq.view(torch.uint8).t().contiguous().view(ops.FP8)
                if train and not lora_site and n not in P.qt:        # fp8_dgrad: nothing reads a bf16 transpose of those Linears
                    P.wt[n] = ops.transpose(w)
    model._packed, model._packed_version = P, ver
    return P


def _packed_lora(model: HunyuanBlocks) -> SimpleNamespace:
    """per adapted Linear: W_ext [N, D + EXT] = [W | scaling B (block structure: adapter j in columns j r .. of its row block) | 0], its
    transpose, A3 [EXT, D] (rows j r ..: A_j) and its transpose -- the K-extension of DESIGN 3 "LoRA as a K-extension", so that
    y = [x | x A3^T] W_ext^T is ONE GEMM with the Linear's own epilogue.  Rebuilt when the adapters change (optimizer step)."""
    L = model.lora
    ver = -1 if L.train_state is None else L.train_state.version
    if L._packed is not None and L._packed_version == ver:
        return L._packed
    if L.wide:
        return _packed_lora_wide(model, ver)
    # The frozen base weight fills all but 64 columns of W_ext: when only the ADAPTERS changed (an optimizer step in LoRA mode: the base weights'
    # version stands still) the previous W_ext / W_ext^T are kept and only their extension columns / rows are rewritten -- re-copying and
    # re-transposing 3072 x 9216 base weights per site and step was 9 ms of the step.
    base_key = (id(_packed_hy(model)), model.fp8, model.fp8_dgrad)             # a new base pack (weights loaded / trained / fp8 switched) invalidates the copies
    prev = L._packed if (L._packed is not None and getattr(L, "_packed_base", None) == base_key) else None
    D, r = L.D, L.r
    dev = L.flat_bf16.device
    # fp8_dgrad: the base dX product reads the fp8 transposed weight (_packed_hy's qt), so W_ext^T keeps only its EXT extension rows
    # (scaling B^T, for dt = g (scaling B)); `to` = the first extension row of the W_ext^T stacks
    to = 0 if (model.fp8 == "mfma" and model.fp8_dgrad) else D
    if prev is None:
        # Stacked storage: the modules with three adapters (qkv / linear1) and those with one (proj) live in two arrays each, so that the
        # per-step refresh of the extension columns and the gradient scatter are a handful of batched kernels instead of six tiny ones per
        # adapter (200 adapters: ~1 800 launches a step).  The per-module operands handed to the GEMMs are views of the stacks.
        P = SimpleNamespace(wext={}, wtext={}, a3={}, a3t={}, db={}, da={})
        mods3 = [m_ for m_, t_ in L.sites.items() if len(t_) == 3]
        mods1 = [m_ for m_, t_ in L.sites.items() if len(t_) == 1]
        assert len(mods3) + len(mods1) == len(L.sites)
        P.mods3, P.mods1 = mods3, mods1
        site_of, sidx = {}, 0
        regular = True                                          # adapter s occupies [2 s r D, 2 (s + 1) r D) of the flat buffers: A_s then B_s
        for mod, tags in L.sites.items():
            for t in tags:
                dot = "." + t if t else ""
                regular &= L.offsets[f"{mod}.lora_A{dot}.weight"] == 2 * sidx * r * D and L.offsets[f"{mod}.lora_B{dot}.weight"] == (2 * sidx + 1) * r * D
                site_of[(mod, t)] = sidx
                sidx += 1
        P.nsites, P.regular = sidx, bool(regular)        # the feed-forward sites' parameters lie behind these 2 sidx r D elements
        P.idx3 = [torch.tensor([site_of[(m_, t)] for m_ in mods3], dtype=torch.long, device=dev) for t in ("q", "k", "v")]
        P.idx1 = torch.tensor([site_of[(m_, "")] for m_ in mods1], dtype=torch.long, device=dev)
        n3, n1 = len(mods3), len(mods1)
        P.W3 = torch.zeros(n3, 3 * D, D + EXT, dtype=BF16, device=dev); P.WT3 = torch.zeros(n3, to + EXT, 3 * D, dtype=BF16, device=dev)
        P.W1 = torch.zeros(n1, D, D + EXT, dtype=BF16, device=dev); P.WT1 = torch.zeros(n1, to + EXT, D, dtype=BF16, device=dev)
        P.A3 = torch.zeros(n3 + n1, EXT, D, dtype=BF16, device=dev); P.A3T = torch.zeros(n3 + n1, D, EXT, dtype=BF16, device=dev)
        P.DB3 = torch.zeros(n3, 3 * D, EXT, dtype=F32, device=dev); P.DB1 = torch.zeros(n1, D, EXT, dtype=F32, device=dev)      # gradient staging (fp32)
        P.DA = torch.zeros(n3 + n1, EXT, D, dtype=F32, device=dev)
        with torch.no_grad():
            for grp, (mods, Wst, WTst, DBst) in enumerate(((mods3, P.W3, P.WT3, P.DB3), (mods1, P.W1, P.WT1, P.DB1))):
                for i, mod in enumerate(mods):
                    nrows = D * len(L.sites[mod])                           # linear1: only its first 3 D rows (q | k | v) are adapted
                    w = _packed_hy(model).w.get(mod + ".weight")            # fp8 mode: the de-quantised E4M3 weight
                    if w is None:
                        w = model.flat(model.flat_bf16, mod + ".weight")
                    Wst[i][:, :D] = w[:nrows]
                    if to:
                        WTst[i][:D] = ops.transpose(w[:nrows])
                    k = i + (0 if grp == 0 else n3)
                    P.wext[mod], P.wtext[mod], P.a3[mod], P.a3t[mod] = Wst[i], WTst[i], P.A3[k], P.A3T[k]
                    P.db[mod], P.da[mod] = DBst[i], P.DA[k]
    else:
        P = prev
    n3 = len(P.mods3)
    with torch.no_grad():
        if P.regular:
            S2 = L.flat_bf16[:2 * P.nsites * r * D].view(P.nsites, 2, r * D)
            A_all = S2[:, 0].reshape(P.nsites, r, D)
            sB_all = (S2[:, 1].float() * L.scaling).to(BF16).view(P.nsites, D, r)                  # scaling B, [D, r] per adapter
            for j in range(3):
                sb, a = sB_all[P.idx3[j]], A_all[P.idx3[j]]                                       # [n3, D, r], [n3, r, D]
                P.W3[:, j * D:(j + 1) * D, D + j * r:D + (j + 1) * r] = sb
                P.WT3[:, to + j * r:to + (j + 1) * r, j * D:(j + 1) * D] = sb.transpose(1, 2)
                P.A3[:n3, j * r:(j + 1) * r] = a
                P.A3T[:n3, :, j * r:(j + 1) * r] = a.transpose(1, 2)
            if len(P.mods1):
                sb, a = sB_all[P.idx1], A_all[P.idx1]
                P.W1[:, :, D:D + r] = sb
                P.WT1[:, to:to + r] = sb.transpose(1, 2)
                P.A3[n3:, :r] = a
                P.A3T[n3:, :, :r] = a.transpose(1, 2)
        else:                                                       # irregular flat layout (r D not a multiple of 8): adapter by adapter
            for mod, tags in L.sites.items():
                wext, wtext, a3, a3t = P.wext[mod], P.wtext[mod], P.a3[mod], P.a3t[mod]
                for j, t in enumerate(tags):
                    dot = "." + t if t else ""
                    sb = (L._plist[f"{mod}.lora_B{dot}.weight"].float() * L.scaling).to(BF16)          # [D, r]
                    wext[j * D:(j + 1) * D, D + j * r:D + (j + 1) * r] = sb
                    wtext[to + j * r:to + (j + 1) * r, j * D:(j + 1) * D] = sb.t()
                    a = L._plist[f"{mod}.lora_A{dot}.weight"]                                           # [r, D]
                    a3[j * r:(j + 1) * r] = a
                    a3t[:, j * r:(j + 1) * r] = a.t()
    _pack_ff(model, P, prev is None)
    L._packed_base = base_key
    L._packed, L._packed_version = P, ver
    return P


def _packed_lora_wide(model: HunyuanBlocks, ver: int) -> SimpleNamespace:
    """_packed_lora for the wide layout (lora_layout: 3 r > 64 or VT355_LORA_WIDE=1).  Per adapted Linear of n adapters and ext = L.ext_of(mod)
    extension columns: W_ext [n D, D + ext] and W_ext^T [D + ext, n D] (fp8_dgrad: its ext extension rows only) with scaling B_j in rows
    [j D, (j + 1) D) x extension columns [j rp, j rp + r) and zeros in every other extension element, written by vt_lora_pack_b(t)_wide;
    the adapters' A rows stacked [n r, D] (the operand of vt_lora_down_wide / vt_lora_up_add_wide); under fp8_dgrad also A3^T [D, ext]
    (column j rp + i = row i of A_j), the bf16 tail operand of the fp8 dX product.  There are no gradient staging stacks: the rank
    gradients go straight into the adapters' flat fp32 gradient (vt_lora_tn_wide).  As in the narrow layout the frozen base columns are
    kept when only the adapters changed."""
    L = model.lora
    base_key = (id(_packed_hy(model)), model.fp8, model.fp8_dgrad)
    prev = L._packed if (L._packed is not None and getattr(L, "_packed_base", None) == base_key) else None
    D, r, rp = L.D, L.r, L.rp
    dev = L.flat_bf16.device
    dg = model.fp8 == "mfma" and bool(model.fp8_dgrad)
    to = 0 if dg else D
    with torch.no_grad():
        if prev is None:
            P = SimpleNamespace(wext={}, wtext={}, a={}, a3t={}, regular=True)         # regular: nothing is left for lora_scatter
            for mod, tags in L.sites.items():
                n, ext = len(tags), L.ext_of(mod)
                w = _packed_hy(model).w.get(mod + ".weight")                # fp8 mode: the de-quantised E4M3 weight
                if w is None:
                    w = model.flat(model.flat_bf16, mod + ".weight")
                P.wext[mod] = torch.empty(n * D, D + ext, dtype=BF16, device=dev)
                P.wext[mod][:, :D] = w[:n * D]                              # linear1: only its first 3 D rows (q | k | v) are adapted
                P.wtext[mod] = torch.empty(to + ext, n * D, dtype=BF16, device=dev)
                if to:
                    P.wtext[mod][:D] = ops.transpose(w[:n * D])
                P.a[mod] = torch.empty(n * r, D, dtype=BF16, device=dev)
                if dg:
                    P.a3t[mod] = torch.zeros(D, ext, dtype=BF16, device=dev)
        else:
            P = prev
        for mod, tags in L.sites.items():
            n, ext = len(tags), L.ext_of(mod)
            dots = ["." + t if t else "" for t in tags]
            A = [L._plist[f"{mod}.lora_A{d}.weight"] for d in dots]
            torch.cat(A, 0, out=P.a[mod])
            # the pack kernels take the adapters' B stacked [n D, r] in fp32: the bf16 compute copy widened (exact), so that a model loaded
            # from a state dict packs the same bits as the one that trained them
            bcat = torch.cat([L._plist[f"{mod}.lora_B{d}.weight"] for d in dots], 0).float()
            ops.lora_pack_b_wide(bcat, P.wext[mod][:, D:], D + ext, n, D, r, rp, ext, L.scaling)        # the whole extension, zeros included
            ops.lora_pack_bt_wide(bcat, P.wtext[mod][to:], n * D, n, D, r, rp, ext, L.scaling)
            if dg:
                for j, a in enumerate(A):
                    P.a3t[mod][:, j * rp:j * rp + r] = a.t()
    _pack_ff(model, P, prev is None)
    L._packed_base = base_key
    L._packed, L._packed_version = P, ver
    return P


def _pack_ff(model: HunyuanBlocks, P: SimpleNamespace, fresh: bool):
    """the operands of the feed-forward sites (_HYLora.ff), either layout, into P.ff[key].  Per site of in / out widths K / N and ext
    extension columns, the one adapter in extension columns [0, r):
      wext [N, K + ext]   the forward operand [W | scaling B | 0]; linear1's MLP rows: [scaling B | 0 | W], its input buffer carries this
                          site's extension in FRONT of x (the columns behind x belong to the q | k | v product).  fp8="mfma": the extension
                          columns alone (wb, the bf16 tail of vt_gemm_mxfp8)
      sbt  [ext, N]       (scaling B)^T, the operand of dt = g (scaling B)
      wtx  [K, N + ext]   [W^T | A^T | 0], the operand of the input-gradient product over the extended gradient [g | dt] -- the adapter's
                          dX term sits inside the product, in front of its dGELU / residual epilogue.  fp8_dgrad: the A^T columns alone
                          (a3t, the bf16 tail of vt_gemm_mxfp8_dx)
      a    [ext, K]       A over zero rows, the operand of t = x A^T: a bf16 GEMM with N = ext, which writes the extension's zeros too
                          (at K = 12288 / 15360 it runs at twice the rate of vt_lora_down_wide, whose one block per 64 rows walks all of K)
    The frozen base columns are kept when only the adapters changed (fresh = False)."""
    L = model.lora
    if not L.ff:
        return
    r, rpf, ext = L.r, L.rpf, L.ext_ff
    dev = L.flat_bf16.device
    mfma = model.fp8 == "mfma"
    dg = mfma and bool(model.fp8_dgrad)
    with torch.no_grad():
        if fresh:
            P.ff = {}
            for key, s in L.ff.items():
                K, N = s.din, s.dout
                F = SimpleNamespace(wext=None, wtx=None)
                w = _packed_hy(model).w.get(s.mod + ".weight")             # fp8 mode: the de-quantised E4M3 weight
                if w is None:
                    w = model.flat(model.flat_bf16, s.mod + ".weight")
                w = w[s.row0:s.row0 + N]
                front = s.tag == "mlp"
                F.xoff, F.eoff = (ext, 0) if front else (0, K)
                if mfma:
                    F.wb = torch.empty(N, ext, dtype=BF16, device=dev)
                else:
                    F.wext = torch.empty(N, K + ext, dtype=BF16, device=dev)
                    F.wext[:, F.xoff:F.xoff + K] = w
                    F.wb = F.wext[:, F.eoff:F.eoff + ext]
                F.sbt = torch.empty(ext, N, dtype=BF16, device=dev)
                if dg:
                    F.a3t = torch.zeros(K, ext, dtype=BF16, device=dev)
                else:
                    F.wtx = torch.zeros(K, N + ext, dtype=BF16, device=dev)
                    F.wtx[:, :N] = ops.transpose(w)
                    F.a3t = F.wtx[:, N:]
                F.a = torch.zeros(ext, K, dtype=BF16, device=dev)
                P.ff[key] = F
        for key, s in L.ff.items():
            F = P.ff[key]
            a = L._plist[s.a_name]
            F.a[:r].copy_(a)
            F.a3t[:, :r] = a.t()
            b32 = L._plist[s.b_name].float()                               # as _packed_lora_wide: the bf16 compute copy widened (exact)
            ops.lora_pack_b_wide(b32, F.wb, F.wb.stride(0), 1, s.dout, r, rpf, ext, L.scaling)        # the whole extension, zeros included
            ops.lora_pack_bt_wide(b32, F.sbt, s.dout, 1, s.dout, r, rpf, ext, L.scaling)


class _HYRun(_STRun):
    def __init__(self, model: HunyuanBlocks, save: bool):
        self.m, self.save = model, save
        self.P = _packed_hy(model)
        self.fb = model.flat_bf16
        self.ts = model.train_state
        self.tape = []
        self.dev = model.device
        self.lora = model.lora
        self.LP = _packed_lora(model) if model.lora is not None else None
        self.lts = None if model.lora is None else model.lora.train_state
        self.need_dvec = True       # set by _HYFn: does anyone consume d(vec)?
        self._lora_ran = set()      # adapted Linears whose backward has filled its gradient staging slots
        self.sp = model.sp_group
        self.spP = 1
        if self.sp is not None:
            import torch.distributed as dist
            self.spP = dist.get_world_size(self.sp)
        self.q8 = model.fp8 == "mfma"   # fp8="mfma": block Linears' forward on vt_gemm_mxfp8
        self.q8s = None                 # (amax, history, scale) of the activation sites, set by forward()
        self.jit = False                # no history yet: every site scales just in time
        self.dg = self.q8 and bool(model.fp8_dgrad)         # fp8_dgrad: the dX products on vt_gemm_mxfp8_dx
        self.gdt, self.gfmax = (ops.FP8, 448.0) if model.fp8_grad_format == "e4m3" else (ops.FP8_E5M2, 57344.0)
        self.g8s = None                 # (amax, history, scale) of the gradient sites, set by backward()
        self.gjit = False
        # lora_dropout > 0 and model.training: (p, seed) of this forward's keep masks, else None -- and then nothing below is dropout's
        self.drop = lora_dropout_seed(model) if (model.lora is not None and model.lora.p > 0) else None
        if self.drop is not None and self.sp is not None and model.lora_dropout_seed is None:
            raise RuntimeError("lora_dropout under sequence parallelism: every rank of the group must use one mask seed -- set "
                               "model.lora_dropout_seed (HunyuanVideoFlow.training_step broadcasts one per step)")

    # ---- lora_dropout: adapter sites and origin maps (DESIGN 4 "mask convention") ----
    def origin(self, joint: bool, K_log: int, k0: int = 0):
        """the origin map (ops.lora_*_drop_at) of an operand whose rows are this run's image rows (double blocks) or its [image; text]
        rows (joint: single blocks) and whose columns are k0 .. of the adapter's K_log wide input: the mask is keyed by the row of the
        UNSHARDED run, b Li + l resp. b (Li + Lt) + l with the image rows first -- under sequence parallelism this rank's image rows
        start at _sp_rows' first row, the replicated text rows sit behind all of the image rows"""
        Lil, Lt = self._Lil, self._Lt
        Li = Lil * self.spP
        lo = self.m._sp_rows(Li)[0]
        if joint:
            return (Lil + Lt, Li + Lt, Lil, lo, Li - Lil, k0, K_log)
        return (Lil, Li, 0, 0, lo, k0, K_log)

    def drop_down(self, x, a, n: int, r: int, rp: int, ext: int, t, K: int, site0: int, og):
        """t = the adapters' masked down-projections of x (the whole extension, zeros included): one vt_lora_down_wide_drop_at call where
        the n masked copies of an x block fit the LDS, else the largest groups that do (rank 128: one adapter per call)"""
        p, seed = self.drop
        j = 0
        while j < n:
            g = n - j
            while g > 1 and not ops.lora_down_wide_drop_fits(g, rp):
                g -= 1
            last = j + g == n
            ops.lora_down_wide_drop_at(x, a[j * r:], g, r, rp, ext - j * rp if last else g * rp, t[:, j * rp:], K, p, seed, site0 + j, og)
            j += g

    # ---- fp8="mfma": activation sites and their delayed scales ----
    def qsite(self, site):
        """(scale, amax) of activation site `site`: 1-element device views.  Within a forward the scale is fixed"""
        st = self.q8s
        return st.scale[site:site + 1], st.amax[site:site + 1]

    def steady(self, site):
        """(scale, amax) for a PRODUCER to write the site's fp8 copy with, or None when the site scales just in time"""
        return None if (site is None or self.jit) else self.qsite(site)

    def fp8_in(self, site, x, xq=None, copy=None, rows=None, M=None):
        """the e4m3 input of site `site`: xq when its producer already wrote it, else cast from the bf16 x (rows / copy: vt_cast_fp8_scaled's
        row map and bf16 copy).  Just in time (no history): an amax pass, the site's scale from that amax (which seeds its history), the cast"""
        if xq is not None:
            return xq
        scale, amax = self.qsite(site)
        y = torch.empty(x.shape[0] if M is None else M, x.shape[1], dtype=ops.FP8, device=self.dev)
        if self.jit:
            ops.cast_fp8_scaled(x, y, scale, amax, copy=copy, rows=rows)
            st = self.q8s
            ops.fp8_scale_update(amax, st.history[site:site + 1], scale)
            copy = None
        ops.cast_fp8_scaled(x, y, scale, amax, copy=copy, rows=rows)
        return y

    # ---- fp8_dgrad: gradient sites ----
    def gsite(self, site):
        st = self.g8s
        return st.scale[site:site + 1], st.amax[site:site + 1]

    def gsteady(self, site):
        """(scale, amax) for a PRODUCER to write the gradient site's fp8 copy with, or None when the site scales just in time"""
        return None if self.gjit else self.gsite(site)

    def grad_in(self, site, g, gq=None):
        """the quantised gradient of site `site`: gq when its producer already wrote it, else cast from the bf16 g (just in time: amax pass,
        scale from that amax -- which seeds the history --, cast; as fp8_in)"""
        if gq is not None:
            return gq
        scale, amax = self.gsite(site)
        y = torch.empty(g.shape[0], g.shape[1], dtype=self.gdt, device=self.dev)
        if self.gjit:                   # once per reset, as fp8_in: this first cast serves as the amax pass (what it writes to y is overwritten)
            ops.cast_fp8_fmt(g, y, scale, amax)
            ops.fp8_scale_update_fmax(amax, self.g8s.history[site:site + 1], scale, self.gfmax)
        ops.cast_fp8_fmt(g, y, scale, amax)
        return y

    def gate_mul_q(self, g, gate, bs, N, rps, site, ext: int = 0):
        """(gg, ggq) = g * gate and its quantised copy for gradient site `site`, in one pass once the site has a history (ggq = None
        without fp8_dgrad).  ext > 0 (the gradient of an adapted feed-forward Linear): gg is the first N columns of an [M, N + ext]
        buffer, returned third -- the extended gradient [gg | dt] of ff_rank / ff_dx"""
        M = g.shape[0]
        gge = self.E(M, N + ext) if ext else None
        gg = gge[:, :N] if ext else self.E(M, N)
        if ext:
            return (gg,) + self._gate_mul_q(g, gg, gate, bs, N, rps, site) + (gge,)
        return (gg,) + self._gate_mul_q(g, gg, gate, bs, N, rps, site)

    def _gate_mul_q(self, g, gg, gate, bs, N, rps, site):
        M = g.shape[0]
        q = self.gsteady(site) if self.dg else None
        if q is None:
            ops.gate_mul(g, gg, gate, gate, bs, N, rps, 0)
            return ((self.grad_in(site, gg) if self.dg else None),)
        ggq = torch.empty(M, N, dtype=self.gdt, device=self.dev)
        ops.gate_mul_fp8(g, gg, gate, gate, bs, N, rps, 0, ggq, q[0], q[1])
        return (ggq,)

    def dx_gemm(self, gq, site, wname, dx, rows=None, cols=None, **kw):
        """dx = epilogue((gq WqT^T) s_g s_w) on vt_gemm_mxfp8_dx; rows / cols = (lo, hi): that slice of the transposed weight [K_in, N_out]
        (linear2's column ranges are its rows, linear1's row ranges its columns)"""
        wqt, sw = self.P.qt[wname], self.P.q[wname][1]
        if rows is not None:
            wqt = wqt[rows[0]:rows[1]]
        if cols is not None:
            wqt = wqt[:, cols[0]:cols[1]]
        ops.gemm_mxfp8_dx(gq, wqt, dx, self.gsite(site)[0], sw, **kw)
        return dx

    def dx_dgelu(self, gg, ggq, gsite, usite, wname, du, u, rows=None, ff=None, gge=None):
        """du = (gg W) * gelu'(u) (rows: that row range of the transposed weight).  fp8_dgrad: from the quantised ggq of site `gsite` on the
        fp8 matrix cores, returning the quantised du of site `usite` (written by the epilogue once the site has a history); else bf16, None.
        ff = the key of an adapted feed-forward Linear whose extended gradient is gge = [gg | dt]: du = (gg W + dt A) * gelu'(u), the
        adapter's term inside the product (ff_dx)"""
        if ff is not None:
            q = self.gsteady(usite) if self.dg else None
            duq = None if q is None else torch.empty(du.shape[0], du.shape[1], dtype=self.gdt, device=self.dev)
            kw = {} if q is None else dict(out_fp8=(duq, q[0], q[1]))
            self.ff_dx(ff, gge, du, ggq, gsite, wname, rows=rows, epilogue=EPI_DGELU, pre_act_in=u, **kw)
            return self.grad_in(usite, du, duq) if self.dg else None
        if not self.dg:
            wt = self.P.wt[wname]
            ops.gemm(gg, wt if rows is None else wt[rows[0]:rows[1]], du, None, epilogue=EPI_DGELU, pre_act_in=u)
            return None
        q = self.gsteady(usite)
        duq = None if q is None else torch.empty(du.shape[0], du.shape[1], dtype=self.gdt, device=self.dev)
        self.dx_gemm(ggq, gsite, wname, du, rows=rows, epilogue=EPI_DGELU, pre_act_in=u, out_fp8=None if q is None else (duq, q[0], q[1]))
        return self.grad_in(usite, du, duq)

    def mx_gemm(self, xq, site, wname, y, bias, rows=None, **epi):
        """y = epilogue((xq Wq^T) sa sw + bias) on vt_gemm_mxfp8; rows = (lo, hi): that row range of the weight (linear1)"""
        wq, sw = self.P.q[wname]
        if rows is not None:
            wq = wq[rows[0]:rows[1]]
        ops.gemm_mxfp8(xq, wq, y, self.qsite(site)[0], sw, bias, **epi)
        return y

    def W(self, name):
        """the parameter view, or in fp8 mode the de-quantised E4M3 copy of a block Linear's weight (biases / norm weights stay bf16)"""
        w = self.P.w.get(name)
        return w if w is not None else super().W(name)

    @property
    def mod_grads(self) -> bool:
        """Are the gradients of the modulation vectors (shift / scale / gate) wanted?  Only the modulation Linears' own weights and d(vec)
        consume them; with frozen block weights (LoRA) and a conditioning vector that needs no gradient (the whole model: vec comes out of
        frozen embedders) autograd would not compute them either -- the per-block column sums over g and g * branch, the saved pre-gate
        branches and the modulation Linears' input gradients are skipped."""
        return self.ts is not None or self.need_dvec

    # ---- frozen block weights (LoRA mode: self.ts is None): no gradient buffers, no dW GEMMs ----
    def G(self, name):
        return None if self.ts is None else self.m.flat(self.ts.grad, name)

    def dW(self, dy, x, target):
        if target is not None:
            super().dW(dy, x, target)

    def colsum(self, g, name, D):
        if self.ts is not None:
            ops.group_colsum(g, self.G(name), D=D)

    def ext(self, M, proj: bool = False):
        """activation buffer of an adapted Linear's input: [M, D + ext] (ext: the K-extension of the fused q | k | v projections, or with
        proj=True that of img_attn_proj), the Linear reads all of it, producers write [:, :D]"""
        return self.E(M, self.m.hidden_size + (self.lora.ext_proj if proj else self.lora.ext_qkv))

    def lora_linear(self, xe, mod: str, bias, y=None, q8=None, **epi):
        """y = [x | x A3^T] W_ext^T + bias (+ epilogue) for the adapted Linear `mod`; xe: ext buffer whose [:, :D] holds x.  Returns
        (y, backward(g) -> dx [M, D]) -- the caller decides what g is (gated or not) and where dx goes.  q8 = (xq, site, wname, rows):
        the base product x W^T on vt_gemm_mxfp8 from the e4m3 input, the extension columns as its bf16 tail."""
        if self.lora.wide:
            return self._lora_linear_wide(xe, mod, bias, y, q8, epi)
        D = self.m.hidden_size
        M = xe.shape[0]
        wext, a3 = self.LP.wext[mod], self.LP.a3[mod]
        ops.gemm(xe[:, :D], a3, xe[:, D:], None, K=D)                  # t = x A3^T into the extension columns
        if y is None:
            y = self.E(M, wext.shape[0])
        if q8 is not None:
            xq, site, wname, rows = q8
            self.mx_gemm(xq, site, wname, y, bias, rows=rows, tail=(xe[:, D:], wext[:, D:]), **epi)
        else:
            ops.gemm(xe, wext, y, bias, **epi)

        def backward(g, gq=None, gsite=None):
            L, r = self.lora, self.lora.r
            if self.dg and q8 is not None:
                # dx = (gq WqT^T) s + dt A3: dt = g (scaling B) in bf16, dt A3 through the GEMM's bf16 tail
                dt = self.E(M, EXT)
                ops.gemm(g, self.LP.wtext[mod], dt, None)       # fp8_dgrad: W_ext^T holds its extension rows only
                if self.lts is not None:
                    db, da = self.LP.db[mod], self.LP.da[mod]
                    ops.linear_dw(g, xe[:, D:], db, accumulate=False)
                    ops.linear_dw(dt, xe[:, :D], da, accumulate=False)
                    self._lora_ran.add(mod)
                    if not self.LP.regular:
                        self._lora_scatter_one(mod)
                dx = self.E(M, D)
                self.dx_gemm(self.grad_in(gsite, g, gq), gsite, q8[2], dx, cols=q8[3], tail=(dt, self.LP.a3t[mod]))
                return dx
            assert not self.dg, "fp8_dgrad: every adapted Linear runs on vt_gemm_mxfp8 (W_ext^T holds no base rows)"
            dxe = self.E(M, D + EXT)
            ops.gemm(g, self.LP.wtext[mod], dxe, None)                  # [dx | dt] = g W_ext
            if self.lts is not None:
                db, da = self.LP.db[mod], self.LP.da[mod]               # this module's slots of the gradient staging stacks (overwritten)
                ops.linear_dw(g, xe[:, D:], db, accumulate=False)       # d(scaling B) blocks = g^T t
                ops.linear_dw(dxe[:, D:], xe[:, :D], da, accumulate=False)   # dA3 = dt^T x
                self._lora_ran.add(mod)
                if not self.LP.regular:
                    self._lora_scatter_one(mod)
            dx = self.E(M, D)
            ops.gemm(dxe[:, D:], self.LP.a3t[mod], dx, None, epilogue=EPI_GATED_RES, residual=dxe[:, :D])     # dx + dt A3
            return dx
        return y, backward

    def _lora_linear_wide(self, xe, mod: str, bias, y, q8, epi):
        """lora_linear in the wide layout: the rank-side products on the MFMA kernels of csrc/lora_wide.hip.  t = x A^T of all the
        Linear's adapters in one pass over x (the call writes the whole extension, zeros included); the base product as in the narrow
        layout; backward: the rank gradients of each adapter straight into its slice of the flat fp32 gradient (fp32 atomics: not
        bitwise reproducible from run to run), dx += sum_j dt_j A_j in one pass -- or, under fp8_dgrad, through the bf16 tail of the fp8
        dX product"""
        L, D = self.lora, self.m.hidden_size
        M, ext = xe.shape[0], xe.shape[1] - D
        tags, r, rp = L.sites[mod], L.r, L.rp
        n = len(tags)
        wext, wtext, a = self.LP.wext[mod], self.LP.wtext[mod], self.LP.a[mod]
        assert ext == L.ext_of(mod) and wext.shape[1] == D + ext
        drop = self.drop
        if drop is not None:            # adapter j reads x under the mask of site s0 + j; the rows: image rows, or linear1's [image; text]
            s0 = L.site_of[f"{mod}.lora_A{'.' + tags[0] if tags[0] else ''}.weight"]
            og = self.origin(mod.startswith("single_blocks."), D)
            self.drop_down(xe, a, n, r, rp, ext, xe[:, D:], D, s0, og)
        else:
            ops.lora_down_wide(xe, a, n, r, rp, ext, xe[:, D:], D)
        if y is None:
            y = self.E(M, wext.shape[0])
        if q8 is not None:
            xq, site, wname, rows = q8
            self.mx_gemm(xq, site, wname, y, bias, rows=rows, tail=(xe[:, D:], wext[:, D:]), **epi)
        else:
            ops.gemm(xe, wext, y, bias, **epi)

        def backward(g, gq=None, gsite=None):
            fp8dx = self.dg and q8 is not None
            assert fp8dx or not self.dg, "fp8_dgrad: every adapted Linear runs on vt_gemm_mxfp8 (W_ext^T holds no base rows)"
            if fp8dx:
                dt = self.E(M, ext)
                ops.gemm(g, wtext, dt, None)                            # dt = g (scaling B): W_ext^T holds its extension rows only
            else:
                dxe = self.E(M, D + ext)
                ops.gemm(g, wtext, dxe, None)                           # [dx | dt] = g W_ext
                dt = dxe[:, D:]
            if self.lts is not None:
                for j, t in enumerate(tags):
                    dot = "." + t if t else ""
                    gB = L.flat(self.lts.grad, f"{mod}.lora_B{dot}.weight")         # [D, r]
                    gA = L.flat(self.lts.grad, f"{mod}.lora_A{dot}.weight")         # [r, D]
                    ops.lora_tn_wide(g[:, j * D:(j + 1) * D], xe[:, D + j * rp:], r, gB, r, 1, L.scaling, D)    # dB_j += scaling g_j^T t_j
                    if drop is not None:                                                                        # dA_j += dt_j^T (keep_j * x) / (1 - p)
                        ops.lora_tn_wide_drop_at(xe[:, :D], dt[:, j * rp:], r, gA, 1, D, 1.0, D, drop[0], drop[1], s0 + j, og)
                    else:
                        ops.lora_tn_wide(xe[:, :D], dt[:, j * rp:], r, gA, 1, D, 1.0, D)                        # dA_j += dt_j^T x
            if fp8dx:
                dx = self.E(M, D)
                self.dx_gemm(self.grad_in(gsite, g, gq), gsite, q8[2], dx, cols=q8[3], tail=(dt, self.LP.a3t[mod]))
                return dx
            if drop is not None:                                        # dx += sum_j keep_j * (dt_j A_j) / (1 - p), in place
                ops.lora_up_add_wide_drop_at(dxe, dt, a, n, r, rp, D, drop[0], drop[1], s0, og)
            else:
                ops.lora_up_add_wide(dxe, dt, a, n, r, rp, D)           # dx += sum_j dt_j A_j, in place
            return dxe[:, :D]                                           # a row-strided view
        return y, backward

    # ---- the feed-forward sites (_HYLora.ff, _pack_ff): one adapter each, either layout ----
    def ff_key(self, key: str):
        """key when `key` names an adapted feed-forward site, else None"""
        return key if (self.lora is not None and key in self.lora.ff) else None

    def ff_forward(self, key: str, buf, y, bias, q8=None, **epi):
        """y = epilogue([x | x A^T] [W | scaling B]^T + bias) for the feed-forward site `key`; buf: the site's input buffer, x in the
        columns [xoff, xoff + K) and the extension, written here (t = x A^T, zeros past the rank), in [eoff, eoff + ext)
        (_pack_ff).  q8 = (xq, site, wname, rows): the base product on vt_gemm_mxfp8, the extension as its bf16 tail.  Returns (x, t)."""
        L, F = self.lora, self.LP.ff[key]
        s = L.ff[key]
        K, ext = s.din, L.ext_ff
        x, t = buf[:, F.xoff:F.xoff + K], buf[:, F.eoff:F.eoff + ext]
        if self.drop is not None:       # t = (keep * x) A^T / (1 - p): the site's own mask over its whole input
            self.drop_down(x, F.a, 1, L.r, L.rpf, ext, t, K, L.site_of[s.a_name], self.ff_origin(key))
        else:
            ops.gemm(x, F.a, t, None)
        if q8 is not None:
            xq, site, wname, rows = q8
            self.mx_gemm(xq, site, wname, y, bias, rows=rows, tail=(t, F.wb), **epi)
        else:
            ops.gemm(buf[:, :K + ext], F.wext, y, bias, **epi)
        return x, t

    def ff_origin(self, key: str, k0: int = 0):
        """origin map of the feed-forward site `key` (columns k0 .. of its input): the single blocks' sites see [image; text] rows"""
        return self.origin(key.startswith("single_blocks."), self.lora.ff[key].din, k0)

    def ff_rank(self, key: str, ge, x, t):
        """the rank side of site `key`'s backward: ge = [g | .] the extended output gradient, x / t the site's input and t = x A^T.
        dt = g (scaling B) into ge's extension columns, then the adapter's gradients straight into its slices of the flat fp32 gradient
        (vt_lora_tn_wide: fp32 atomics, nothing staged -- a partial backward touches what it reaches)."""
        L, F = self.lora, self.LP.ff[key]
        s = L.ff[key]
        N = s.dout
        g, dt = ge[:, :N], ge[:, N:N + L.ext_ff]
        ops.gemm(g, F.sbt, dt, None)
        if self.lts is not None:
            ops.lora_tn_wide(g, t, L.r, L.flat(self.lts.grad, s.b_name), L.r, 1, L.scaling, N)           # dB += scaling g^T t
            if self.drop is not None:                                                                    # dA += dt^T (keep * x) / (1 - p)
                ops.lora_tn_wide_drop_at(x, dt, L.r, L.flat(self.lts.grad, s.a_name), 1, s.din, 1.0, s.din, self.drop[0], self.drop[1],
                                         L.site_of[s.a_name], self.ff_origin(key))
            else:
                ops.lora_tn_wide(x, dt, L.r, L.flat(self.lts.grad, s.a_name), 1, s.din, 1.0, s.din)      # dA += dt^T x

    def ff_dx(self, key: str, ge, out, gq, gsite, wname, rows=None, cols=None, **epi):
        """out = epilogue(g W + dt A) of site `key` from the extended gradient ge = [g | dt] (after ff_rank): ONE product over
        [W^T | A^T], so the adapter's term is in front of a dGELU / residual epilogue; rows = (lo, hi): those input columns (linear2's
        attention and MLP halves).  fp8_dgrad: g W on vt_gemm_mxfp8_dx from the quantised gq of gradient site `gsite` (cols: linear1's
        row range of the fp8 weight), dt A as its bf16 tail."""
        F, N = self.LP.ff[key], self.lora.ff[key].dout
        lo, hi = rows if rows is not None else (0, F.a3t.shape[0])
        if self.drop is not None:
            # lora_dropout: the adapter's term keep * (dt A) / (1 - p) is masked per element of `out` and the base product is not, so it
            # cannot ride in the product: the base product alone with the epilogue, then the masked correction in place -- times
            # gelu'(u) where the epilogue was the dGELU one (the site's input is gelu(u): out = (g W + keep * (dt A) / (1 - p)) gelu'(u))
            L = self.lora
            ops.gemm(ge[:, :N], F.wtx[lo:hi, :N], out, None, **epi)
            og = self.ff_origin(key, k0=lo)
            args = (out, ge[:, N:N + L.ext_ff], F.a[:, lo:hi], 1, L.r, L.rpf)
            if epi.get("epilogue") == EPI_DGELU:
                ops.lora_up_add_wide_dgelu_drop_at(*args, epi["pre_act_in"], hi - lo, self.drop[0], self.drop[1], L.site_of[L.ff[key].a_name], og)
            else:
                ops.lora_up_add_wide_drop_at(*args, hi - lo, self.drop[0], self.drop[1], L.site_of[L.ff[key].a_name], og)
            return out
        if self.dg:
            self.dx_gemm(gq, gsite, wname, out, rows=rows, cols=cols, tail=(ge[:, N:N + self.lora.ext_ff], F.a3t[lo:hi]), **epi)
        else:
            ops.gemm(ge[:, :N + self.lora.ext_ff], F.wtx[lo:hi], out, None, **epi)
        return out

    def _lora_scatter_one(self, mod):
        """staging slots of one module -> its adapters' gradients"""
        L, r, D = self.lora, self.lora.r, self.m.hidden_size
        db, da = self.LP.db[mod], self.LP.da[mod]
        for j, t in enumerate(L.sites[mod]):
            dot = "." + t if t else ""
            L.flat(self.lts.grad, f"{mod}.lora_B{dot}.weight").add_(db[j * D:(j + 1) * D, j * r:(j + 1) * r], alpha=L.scaling)
            L.flat(self.lts.grad, f"{mod}.lora_A{dot}.weight").add_(da[j * r:(j + 1) * r])

    def lora_scatter(self):
        """end of the backward: every adapted Linear has left d(scaling B) / dA3 in the staging stacks -- add them to the adapters' flat
        gradient in a few batched kernels (the flat buffer is [A_0 | B_0 | A_1 | B_1 ...], one [r, D] + [D, r] pair per adapter)"""
        if self.lts is None or self.LP is None or not self.LP.regular or not self._lora_ran:
            return
        P, L = self.LP, self.lora
        if len(self._lora_ran) != len(L.sites):                  # a partial backward: module by module
            for mod in self._lora_ran:
                self._lora_scatter_one(mod)
            self._lora_ran.clear()
            return
        r, D, n3 = L.r, self.m.hidden_size, len(P.mods3)
        G2 = self.lts.grad[:2 * P.nsites * r * D].view(P.nsites, 2, r * D)
        GA, GB = G2[:, 0].view(P.nsites, r, D), G2[:, 1].view(P.nsites, D, r)
        for j in range(3):
            GB.index_add_(0, P.idx3[j], P.DB3[:, j * D:(j + 1) * D, j * r:(j + 1) * r], alpha=L.scaling)
            GA.index_add_(0, P.idx3[j], P.DA[:n3, j * r:(j + 1) * r])
        if len(P.mods1):
            GB.index_add_(0, P.idx1, P.DB1[:, :, :r], alpha=L.scaling)
            GA.index_add_(0, P.idx1, P.DA[n3:, :r])
        self._lora_ran.clear()

    def linear(self, x: _Var, wname: str, bname, residual=None, wspan=None, out=None, site=None, xq=None, gsite=None) -> _Var:
        """block Linear without epilogue (the qkv projections).  Adapted module (LoRA): one GEMM over the K-extended operands.  fp8=True: the
        FORWARD product on the fp8 matrix cores (activation quantised per tensor here, weight copy + scale from _packed_hy).  Parameter
        gradients only when the block weights train."""
        assert residual is None and wspan is None and out is None
        mod = wname[:-7]
        M = x.d.shape[0]
        b = None if bname is None else self.W(bname)
        mx = self.q8 and wname in self.P.q
        if mx:
            xq = self.fp8_in(site, x.d, xq)
        if self.lora is not None and mod in self.lora.sites:
            y, bw = self.lora_linear(x.ext, mod, b, q8=(xq, site, wname, None) if mx else None)
            yv = _Var(y)
            if self.save:
                def bwd_linear_lora():
                    self.colsum(yv.g, bname, y.shape[1])
                    gq, yv.gq = yv.gq, None
                    self.acc(x, bw(yv.g, gq, gsite))
                self.tape.append(bwd_linear_lora)
            return yv
        w = self.W(wname)
        y = self.E(M, w.shape[0])
        if mx:
            self.mx_gemm(xq, site, wname, y, b)
        elif self.m.fp8 and wname in self.P.q:
            wq, sw = self.P.q[wname]
            xq, sa = ops.quantize_fp8(x.d)
            ops.gemm_fp8(xq, wq, y, sa, sw, b)
        else:
            ops.gemm(x.d, w, y, b)
        yv = _Var(y)
        if self.save:
            def bwd_linear():
                g = yv.g
                self.colsum(g, bname, w.shape[0])
                self.dW(g, x.d, self.G(wname))
                dx = self.E(M, w.shape[1])
                if self.dg and mx:
                    gq, yv.gq = yv.gq, None
                    self.dx_gemm(self.grad_in(gsite, g, gq), gsite, wname, dx)
                else:
                    ops.gemm(g, self.P.wt[wname], dx, None)
                self.acc(x, dx)
            self.tape.append(bwd_linear)
        return yv

    def ln_mod(self, x: _Var, shift, scale, bstride: int, rows_per_sample: int, dshift, dscale, dbstride: int, ext: bool = False, site=None):
        """as _STRun.ln_mod; ext=True: the result is written into the first D columns of an extended buffer (input of an adapted Linear).
        site given (fp8="mfma"): returns (y, yq) -- yq the e4m3 copy of y for that activation site (None while it scales just in time)"""
        q = self.steady(site) if self.q8 else None
        if not ext and q is None:
            yv = super().ln_mod(x, shift, scale, bstride, rows_per_sample, dshift, dscale, dbstride)
            return yv if site is None else (yv, None)
        M, D = x.d.shape
        # ext = (front, back): extension columns in front of / behind the D columns of y (feed-forward sites; True: the q | k | v extension)
        front, back = ext if isinstance(ext, tuple) else (0, self.lora.ext_qkv if ext else 0)
        buf = self.E(M, front + D + back) if ext else None
        y = buf[:, front:front + D] if ext else self.E(M, D)
        mean, rstd = self.E(M, dt=F32), self.E(M, dt=F32)
        yq = None
        if q is not None:
            yq = torch.empty(M, D, dtype=ops.FP8, device=self.dev)
            ops.ln_modulate_fwd_fp8(x.d, y, None, None, (shift, scale, shift, scale, bstride), mean, rstd, D, rows_per_sample, 0, 1e-6,
                                    yq, q[0], q[1])
        else:
            ops.ln_modulate_fwd(x.d, y, None, None, (shift, scale, shift, scale, bstride), mean, rstd, D, rows_per_sample, 0, 1e-6)
        yv = _XVar(y, buf) if ext else _Var(y)
        if self.save:
            def bwd_ln_mod_ext():
                g = yv.g
                if dshift is not None:
                    ops.group_colsum(g, dshift, y=x.d, out2=dscale, mean=mean, rstd=rstd, D=D, S=rows_per_sample, St=0, grouped=True,
                                     o_bstride=dbstride, o_segstride=0)
                dx = self.E(M, D)
                ops.ln_modulate_bwd(g, x.d, mean, rstd, None, (scale, scale, bstride), x.g, dx, D, rows_per_sample, 0)
                x.g = dx
            self.tape.append(bwd_ln_mod_ext)
        return yv if site is None else (yv, yq)

    def mlp(self, x: _Var, pre: str, residual=None, gate=None, dgate=None, sites=None, xq=None, gsites=None) -> _Var:
        """_STRun.mlp with the parameter gradients behind the frozen-weights switch; fp8="mfma": sites = (fc1 input, fc2 input), xq the
        e4m3 fc1 input (or None), the GELU epilogue of fc1 writing fc2's e4m3 input"""
        M = x.d.shape[0]
        w1, w2 = self.W(pre + "fc1.weight"), self.W(pre + "fc2.weight")
        H4, Dout = w1.shape[0], w2.shape[0]
        # adapted feed-forward sites (LoRA targets ff.net.0.proj / ff.net.2): x lives in an extended buffer (ln_mod ext), ga gets one
        k1, k2 = self.ff_key(pre + "fc1"), self.ff_key(pre + "fc2")
        fext = self.lora.ext_ff if (k1 or k2) else 0
        u = self.E(M, H4)
        gae = self.E(M, H4 + fext) if k2 else None
        ga = gae[:, :H4] if k2 else self.E(M, H4)
        y = self.E(M, Dout)
        branch = self.E(M, Dout) if (self.save and dgate is not None) else None          # the pre-gate branch: only d(gate) reads it
        epi2 = dict(epilogue=EPI_GATED_RES, residual=residual.d, gate_txt=gate[0], gate_vid=gate[0], gate_bstride=gate[1], S=gate[2], St=0,
                    pre_act_out=branch)
        if self.q8:
            s1, s2 = sites
            q2 = self.steady(s2)
            gq = None if q2 is None else torch.empty(M, H4, dtype=ops.FP8, device=self.dev)
            epi1 = dict(epilogue=EPI_BIAS_GELU, pre_act_out=u, out_fp8=None if q2 is None else (gq, q2[0], q2[1]))
            if k1:
                self.ff_forward(k1, x.ext, ga, self.W(pre + "fc1.bias"), q8=(self.fp8_in(s1, x.d, xq), s1, pre + "fc1.weight", None), **epi1)
            else:
                self.mx_gemm(self.fp8_in(s1, x.d, xq), s1, pre + "fc1.weight", ga, self.W(pre + "fc1.bias"), **epi1)
            if k2:
                self.ff_forward(k2, gae, y, self.W(pre + "fc2.bias"), q8=(self.fp8_in(s2, ga, gq), s2, pre + "fc2.weight", None), **epi2)
            else:
                self.mx_gemm(self.fp8_in(s2, ga, gq), s2, pre + "fc2.weight", y, self.W(pre + "fc2.bias"), **epi2)
            del gq
        else:
            if k1:
                self.ff_forward(k1, x.ext, ga, self.W(pre + "fc1.bias"), epilogue=EPI_BIAS_GELU, pre_act_out=u)
            else:
                ops.gemm(x.d, w1, ga, self.W(pre + "fc1.bias"), epilogue=EPI_BIAS_GELU, pre_act_out=u)
            if k2:
                self.ff_forward(k2, gae, y, self.W(pre + "fc2.bias"), **epi2)
            else:
                ops.gemm(ga, w2, y, self.W(pre + "fc2.bias"), **epi2)
        yv = _Var(y)
        if self.save:
            def bwd_mlp():
                g_ = yv.g
                self.acc(residual, g_)
                if dgate is not None:
                    ops.group_colsum(g_, None, y=branch, out2=dgate, D=Dout, S=gate[2], St=0, grouped=True, o_bstride=gate[1], o_segstride=0)
                # fp8_dgrad: gated d(fc2 out) and d(u) are quantised by their producers, both dX products run in fp8
                g2, g1 = gsites if self.dg else (None, None)
                gge = None
                if k2:                  # ff.net.2: the extended gradient [gg | dt], the adapter's dX term inside the dGELU product
                    gg, ggq, gge = self.gate_mul_q(g_, gate[0], gate[1], Dout, gate[2], g2, ext=fext)
                    self.ff_rank(k2, gge, ga, gae[:, H4:])
                else:
                    gg, ggq = self.gate_mul_q(g_, gate[0], gate[1], Dout, gate[2], g2)
                self.colsum(gg, pre + "fc2.bias", Dout)
                self.dW(gg, ga, self.G(pre + "fc2.weight"))
                due = self.E(M, H4 + fext) if k1 else None
                du = due[:, :H4] if k1 else self.E(M, H4)
                duq = self.dx_dgelu(gg, ggq, g2, g1, pre + "fc2.weight", du, u, ff=k2, gge=gge)
                del ggq
                self.colsum(du, pre + "fc1.bias", H4)
                self.dW(du, x.d, self.G(pre + "fc1.weight"))
                dx = self.E(M, w1.shape[1])
                if k1:                  # ff.net.0.proj: dx = du W1 + dt A in one product over [du | dt]
                    self.ff_rank(k1, due, x.d, x.ext[:, w1.shape[1]:])
                    self.ff_dx(k1, due, dx, duq, g1, pre + "fc1.weight")
                elif self.dg:
                    self.dx_gemm(duq, g1, pre + "fc1.weight", dx)
                else:
                    ops.gemm(du, self.P.wt[pre + "fc1.weight"], dx, None)
                self.acc(x, dx)
            self.tape.append(bwd_mlp)
        return yv

    def modulation(self, sv: _Var, pre: str, n: int):
        """ModulateDiT (modulate_layers.py:7-27): Linear(SiLU(vec)) -> fp32 [B, n*D]; returns (mod, dmod); sv = SiLU(vec) bf16"""
        B, D = sv.d.shape
        mod = self.E(B, n * D, dt=F32)
        ops.gemm(sv.d, self.W(pre + ".linear.weight"), mod, self.W(pre + ".linear.bias"))
        dmod = torch.zeros(B, n * D, dtype=F32, device=self.dev) if (self.save and self.mod_grads) else None
        if dmod is not None:
            def bwd_modulation():
                ops.small_linear_bwd(dmod, sv.d, self.W(pre + ".linear.weight"), self.G(pre + ".linear.weight"), self.G(pre + ".linear.bias"), self._dsv)
            self.tape.append(bwd_modulation)
        return mod, dmod

    def glinear(self, x: _Var, wname: str, bname: str, residual: _Var, gate, dgate, rps: int, bs: int, site=None, xq=None, gsite=None) -> _Var:
        """y = residual + gate[b] * (x W^T + b)   (apply_gate, modulate_layers.py:49-66); adapted module: over the K-extended operands.
        fp8="mfma": the product from the e4m3 input xq of activation site `site`"""
        mod = wname[:-7]
        adapted = self.lora is not None and mod in self.lora.sites
        w = self.W(wname)
        M, N = x.d.shape[0], w.shape[0]
        y = self.E(M, N)
        branch = self.E(M, N) if (self.save and dgate is not None) else None           # the pre-gate branch: only d(gate) reads it
        epi = dict(epilogue=EPI_GATED_RES, residual=residual.d, gate_txt=gate, gate_vid=gate, gate_bstride=bs, S=rps, St=0, pre_act_out=branch)
        bw = None
        mx = self.q8 and wname in self.P.q
        if adapted:
            y, bw = self.lora_linear(x.ext, mod, self.W(bname), y=y, q8=(xq, site, wname, None) if mx else None, **epi)
        elif mx:
            self.mx_gemm(xq, site, wname, y, self.W(bname), **epi)
        else:
            ops.gemm(x.d, w, y, self.W(bname), **epi)
        yv = _Var(y)
        if self.save:
            def bwd_glinear():
                g_ = yv.g
                self.acc(residual, g_)
                if dgate is not None:
                    ops.group_colsum(g_, None, y=branch, out2=dgate, D=N, S=rps, St=0, grouped=True, o_bstride=bs, o_segstride=0)
                gg, ggq = self.gate_mul_q(g_, gate, bs, N, rps, gsite)
                self.colsum(gg, bname, N)
                if adapted:
                    self.acc(x, bw(gg, ggq, gsite))
                else:
                    self.dW(gg, x.d, self.G(wname))
                    dx = self.E(M, w.shape[1])
                    if ggq is not None:
                        self.dx_gemm(ggq, gsite, wname, dx)
                    else:
                        ops.gemm(gg, self.P.wt[wname], dx, None)
                    self.acc(x, dx)
            self.tape.append(bwd_glinear)
        return yv

    def qkv_to_joint(self, qkv: _Var, pre_q: str, pre_k: str, joint, djoint_ref, L: int, Lj: int, off: int, rope, gsite=None):
        """RMS q/k norm + rope + scatter into the joint [B*Lj, 3C] buffer; backward reads the joint gradient buffer djoint_ref[0]"""
        H = self.m.heads_num
        M = qkv.d.shape[0]
        rstd = self.E(M, 2 * H, dt=F32)
        gq, gk = self.W(pre_q), self.W(pre_k)
        ops.qk_rmsnorm_rope128_fwd(qkv.d, joint, gq, gk, rstd, H, L, Lj, off, rope)
        if self.save:
            def bwd_qkv_to_joint():
                dq = self.E(M, qkv.d.shape[1])
                ops.qk_rmsnorm_rope128_bwd(djoint_ref[0], qkv.d, dq, gq, gk, rstd, self.G(pre_q), self.G(pre_k), H, L, Lj, off, rope)   # frozen: None
                qkv.g = dq
                if self.dg:                     # d(qkv): the one gradient site whose producer does not quantise -- one cast pass
                    qkv.gq = self.grad_in(gsite, dq)
            self.tape.append(bwd_qkv_to_joint)

    def joint_attention(self, joint, B: int, Lj: int, kv_len, o_out, djoint_ref):
        """attention over the joint sequence; o_out: [B*Lj, >= C] buffer view (row stride may exceed C); the backward fills djoint_ref[0]"""
        H = self.m.heads_num
        C = H * 128
        o3 = o_out.view(B, Lj, o_out.shape[1]) if o_out.is_contiguous() else o_out.as_strided((B, Lj, C), (Lj * o_out.stride(0), o_out.stride(0), 1))
        scale = 128 ** -0.5
        rows = lambda g: g.view(B, Lj, g.shape[1]) if g.is_contiguous() else g.as_strided((B, Lj, C), (Lj * g.stride(0), g.stride(0), 1))
        ov = _Var(o_out)
        if self.spP > 1:
            # Ulysses: rows <-> heads around the local attention (sp.py); Lj = local image rows + text rows, the attention sees every row
            from . import sp
            Lt = Lj - self._Lil
            geo = (B, self._Lil, Lt, H, 128, self.sp)
            h, S2 = H // self.spP, self._Lil * self.spP + Lt
            c2 = h * 128
            j2 = sp.joint_to_heads(joint, *geo)                                       # [B, S2, 3 c2]
            o2 = self.E(B, S2, c2)
            lse = self.E(B, h, S2, dt=F32)
            ops.attn128_fwd(j2[:, :, :c2], j2[:, :, c2:2 * c2], j2[:, :, 2 * c2:], o2, lse, h, scale, kv_len=kv_len)
            sp.heads_to_rows(o2, o3[:, :, :C], *geo)
            if self.save:
                def bwd_joint_attention_sp():
                    go2 = sp.rows_grad_to_heads(rows(ov.g)[:, :, :C], *geo)
                    dj2 = self.E(B, S2, 3 * c2)
                    ops.attn128_bwd(j2[:, :, :c2], j2[:, :, c2:2 * c2], j2[:, :, 2 * c2:], o2, go2, lse, dj2[:, :, :c2], dj2[:, :, c2:2 * c2],
                                    dj2[:, :, 2 * c2:], h, scale, kv_len=kv_len)
                    djoint_ref[0] = sp.heads_grad_to_joint(dj2, *geo)
                self.tape.append(bwd_joint_attention_sp)
            return ov
        j3 = joint.view(B, Lj, 3 * C)
        lse = self.E(B, H, Lj, dt=F32)
        ops.attn128_fwd(j3[:, :, :C], j3[:, :, C:2 * C], j3[:, :, 2 * C:], o3[:, :, :C], lse, H, scale, kv_len=kv_len)
        if self.save:
            def bwd_joint_attention():
                g3 = rows(ov.g)
                dj = self.E(B * Lj, 3 * C)
                d3 = dj.view(B, Lj, 3 * C)
                ops.attn128_bwd(j3[:, :, :C], j3[:, :, C:2 * C], j3[:, :, 2 * C:], o3[:, :, :C], g3[:, :, :C], lse, d3[:, :, :C], d3[:, :, C:2 * C],
                                d3[:, :, 2 * C:], H, scale, kv_len=kv_len)        # two-pass backward: dQ, dK, dV straight into the joint gradient
                djoint_ref[0] = dj
            self.tape.append(bwd_joint_attention)
        return ov

    # ------------------------------------------------------------------------------------------------------------------
    def double_block(self, pre: str, img: _Var, txt: _Var, sv: _Var, B, Li, Lt, kv_len, rope, site0: int = 0):
        """site0: the first of this block's 8 fp8 activation sites (per stream img, txt: qkv, proj, fc1, fc2 inputs) and of its 8 gradient
        sites (fp8_dgrad; per stream d(qkv), gated d(proj out), gated d(fc2 out), d(u))"""
        D, H = self.m.hidden_size, self.m.heads_num
        C, Lj = D, Li + Lt
        bs = 6 * D
        joint = self.E(B * Lj, 3 * C)                         # every row is written by the two scatters below
        dj = [None]
        streams = {}
        q8 = self.q8
        for si, (s, x, L, off, rp) in enumerate((("img", img, Li, 0, rope), ("txt", txt, Lt, Li, None))):
            mod, dmod = self.modulation(sv, pre + s + "_mod", 6)
            sl = lambda k, buf=mod: buf[:, k * D:(k + 1) * D]
            dsl = (lambda k, buf=dmod: buf[:, k * D:(k + 1) * D]) if dmod is not None else (lambda k: None)
            adapted = self.lora is not None and self.lora.attn and s == "img"
            qs = site0 + 4 * si                                                     # this stream's qkv / proj / fc1 / fc2 input sites
            if q8:
                xm, xq = self.ln_mod(x, sl(0), sl(1), bs, L, dsl(0), dsl(1), bs, ext=adapted, site=qs)
                qkv = self.linear(xm, pre + s + "_attn_qkv.weight", pre + s + "_attn_qkv.bias", site=qs, xq=xq, gsite=qs)
                del xq
            else:
                xm = self.ln_mod(x, sl(0), sl(1), bs, L, dsl(0), dsl(1), bs, ext=adapted)
                qkv = self.linear(xm, pre + s + "_attn_qkv.weight", pre + s + "_attn_qkv.bias")
            streams[s] = (x, L, off, sl, dsl, qkv, rp, qs)
        # the backward of the scatter must run AFTER the attention's backward has produced the joint gradient: push order = forward order
        for s in ("img", "txt"):
            x, L, off, sl, dsl, qkv, rp, qs = streams[s]
            self.qkv_to_joint(qkv, pre + s + "_attn_q_norm.weight", pre + s + "_attn_k_norm.weight", joint, dj, L, Lj, off, rp, gsite=qs)
        o = self.E(B * Lj, C)
        ov = self.joint_attention(joint, B, Lj, kv_len, o, dj)
        outs = {}
        for s in ("img", "txt"):
            x, L, off, sl, dsl, qkv, rp, qs = streams[s]
            aq = None
            if q8:                          # this stream's rows of the joint output: the bf16 copy and the e4m3 proj input in one pass
                ae = self.ext(B * L, proj=True) if (self.lora is not None and self.lora.attn and s == "img") else None
                ad = ae[:, :C] if ae is not None else self.E(B * L, C)
                aq = self.fp8_in(qs + 1, o, copy=ad, rows=(L, Lj, off), M=B * L)
                av = _XVar(ad, ae) if ae is not None else _Var(ad)
            elif self.lora is not None and self.lora.attn and s == "img":            # input of the adapted projection: extended buffer
                ae = self.ext(B * L, proj=True)
                ae.view(B, L, ae.shape[1])[:, :, :C].copy_(o.view(B, Lj, C)[:, off:off + L])
                av = _XVar(ae[:, :C], ae)
            else:
                av = _Var(o.view(B, Lj, C)[:, off:off + L].reshape(B * L, C))       # this stream's rows of the joint output (a copy)
            if self.save:
                def bwd_split(av=av, off=off, L=L, ov=ov):
                    if ov.g is None:
                        ov.g = self.E(B * Lj, C)              # both streams' splits fill all of it
                    g = av.g                          # row-strided when an adapted projection's wide-layout backward left it
                    ov.g.view(B, Lj, C)[:, off:off + L].copy_(g.view(B, L, C) if g.is_contiguous() else g.as_strided((B, L, C), (L * g.stride(0), g.stride(0), 1)))
                self.tape.append(bwd_split)
            x1 = self.glinear(av, pre + s + "_attn_proj.weight", pre + s + "_attn_proj.bias", x, sl(2), dsl(2), L, bs, site=qs + 1, xq=aq,
                               gsite=qs + 1)
            del aq
            fx = (0, self.lora.ext_ff) if self.ff_key(pre + s + "_mlp.fc1") else False      # ff.net.0.proj: fc1's input in an extended buffer
            if q8:
                hm, hq = self.ln_mod(x1, sl(3), sl(4), bs, L, dsl(3), dsl(4), bs, ext=fx, site=qs + 2)
                outs[s] = self.mlp(hm, pre + s + "_mlp.", residual=x1, gate=(sl(5), bs, L), dgate=dsl(5), sites=(qs + 2, qs + 3), xq=hq,
                                   gsites=(qs + 2, qs + 3))
                del hq
            else:
                hm = self.ln_mod(x1, sl(3), sl(4), bs, L, dsl(3), dsl(4), bs, ext=fx)
                outs[s] = self.mlp(hm, pre + s + "_mlp.", residual=x1, gate=(sl(5), bs, L), dgate=dsl(5))
        return outs["img"], outs["txt"]

    def single_block(self, pre: str, x: _Var, sv: _Var, B, Li, Lt, kv_len, rope, site0: int = 0, gsite0: int = 0):
        """site0: this block's fp8 activation sites (linear1 input, linear2 input = site0 + 1); gsite0: its gradient sites (fp8_dgrad:
        gated d(linear2 out), d(qkv) = gsite0 + 1, d(u) = gsite0 + 2)"""
        D, H = self.m.hidden_size, self.m.heads_num
        M4 = int(D * self.m.ratio)
        Lj = Li + Lt
        M = B * Lj
        bs = 3 * D
        mod, dmod = self.modulation(sv, pre + "modulation", 3)
        sl = lambda k: mod[:, k * D:(k + 1) * D]
        dsl = (lambda k: dmod[:, k * D:(k + 1) * D]) if dmod is not None else (lambda k: None)
        mod1 = pre + "linear1"
        adapted = self.lora is not None and mod1 in self.lora.sites
        # adapted feed-forward sites (LoRA targets proj_mlp / proj_out).  linear1's input feeds two products: the buffer is
        # [MLP adapter's extension | x | q, k, v extension], so that each product reads a contiguous [x | its own extension]
        k1, k2 = self.ff_key(mod1 + "#mlp"), self.ff_key(pre + "linear2")
        fext = self.lora.ext_ff if (k1 or k2) else 0
        front = fext if k1 else 0
        xext = (front, self.lora.ext_qkv if adapted else 0) if (k1 or adapted) else False
        q8 = self.q8
        xq = catq = None
        if q8:
            xm, xq = self.ln_mod(x, sl(0), sl(1), bs, Lj, dsl(0), dsl(1), bs, ext=xext, site=site0)
            xq = self.fp8_in(site0, xm.d, xq)
        else:
            xm = self.ln_mod(x, sl(0), sl(1), bs, Lj, dsl(0), dsl(1), bs, ext=xext)
        w1, b1 = self.W(pre + "linear1.weight"), self.W(pre + "linear1.bias")
        qkv = self.E(M, 3 * D)
        bw1 = None
        if adapted:
            qkv, bw1 = self.lora_linear(xm.ext[:, front:], mod1, b1[:3 * D], y=qkv, q8=(xq, site0, pre + "linear1.weight", (0, 3 * D)) if q8 else None)
        elif q8:
            self.mx_gemm(xq, site0, pre + "linear1.weight", qkv, b1[:3 * D], rows=(0, 3 * D))
        else:
            ops.gemm(xm.d, w1[:3 * D], qkv, b1[:3 * D])
        cate = self.E(M, D + M4 + fext) if k2 else None          # proj_out: linear2's input with its extension columns
        cat = cate[:, :D + M4] if k2 else self.E(M, D + M4)      # [attn | gelu(mlp)], read by linear2
        u = self.E(M, M4)
        if q8:                                                   # the GELU epilogue writes its columns of linear2's e4m3 input
            q2 = self.steady(site0 + 1)
            catq = None if q2 is None else torch.empty(M, D + M4, dtype=ops.FP8, device=self.dev)
            epi1 = dict(epilogue=EPI_BIAS_GELU, pre_act_out=u, out_fp8=None if q2 is None else (catq[:, D:], q2[0], q2[1]))
            if k1:
                self.ff_forward(k1, xm.ext, cat[:, D:], b1[3 * D:], q8=(xq, site0, pre + "linear1.weight", (3 * D, 3 * D + M4)), **epi1)
            else:
                self.mx_gemm(xq, site0, pre + "linear1.weight", cat[:, D:], b1[3 * D:], rows=(3 * D, 3 * D + M4), **epi1)
            del xq
        elif k1:
            self.ff_forward(k1, xm.ext, cat[:, D:], b1[3 * D:], epilogue=EPI_BIAS_GELU, pre_act_out=u)
        else:
            ops.gemm(xm.d, w1[3 * D:], cat[:, D:], b1[3 * D:], epilogue=EPI_BIAS_GELU, pre_act_out=u)
        qkvv = _Var(qkv)
        joint = self.E(M, 3 * D)
        dj = [None]
        catv = _Var(cat)
        if self.save:
            def bwd_linear1():
                du = catv.g[:, D:D + M4]                         # bwd_linear2 left d u = (g W2[:, D:]) * gelu'(u) in the mlp columns
                dqkv = qkvv.g
                if self.ts is not None:
                    gw, gb = self.G(pre + "linear1.weight"), self.G(pre + "linear1.bias")
                    ops.group_colsum(dqkv, gb[:3 * D], D=3 * D); ops.group_colsum(du, gb[3 * D:], D=M4)
                    self.dW(dqkv, xm.d, gw[:3 * D]); self.dW(du, xm.d, gw[3 * D:])
                dqq, duq = qkvv.gq, catv.gq         # fp8_dgrad: left by their producers; both row ranges of linear1 are then
                qkvv.gq = catv.gq = None            # column slices of its transposed fp8 weight
                if adapted:
                    dx = bw1(dqkv, dqq, gsite0 + 1)
                else:
                    dx = self.E(M, D)
                    if self.dg:
                        self.dx_gemm(dqq, gsite0 + 1, pre + "linear1.weight", dx, cols=(0, 3 * D))
                    else:
                        ops.gemm(dqkv, self._wt_rows(pre + "linear1.weight", 0, 3 * D), dx, None)
                dx2 = self.E(M, D)
                if k1:                           # proj_mlp: dx2 = dx + du W1[3D:] + dt A over the extended gradient [du | dt]
                    self.ff_rank(k1, catv.g[:, D:], xm.d, xm.ext[:, :front])
                    self.ff_dx(k1, catv.g[:, D:], dx2, duq, gsite0 + 2, pre + "linear1.weight", cols=(3 * D, 3 * D + M4),
                               epilogue=EPI_GATED_RES, residual=dx)
                elif self.dg:
                    self.dx_gemm(duq, gsite0 + 2, pre + "linear1.weight", dx2, cols=(3 * D, 3 * D + M4), epilogue=EPI_GATED_RES, residual=dx)
                else:
                    ops.gemm(du, self._wt_rows(pre + "linear1.weight", 3 * D, 3 * D + M4), dx2, None, epilogue=EPI_GATED_RES, residual=dx)
                self.acc(xm, dx2)
            self.tape.append(bwd_linear1)
        self.qkv_to_joint(qkvv, pre + "q_norm.weight", pre + "k_norm.weight", joint, dj, Lj, Lj, 0, rope, gsite=gsite0 + 1)
        ov = self.joint_attention(joint, B, Lj, kv_len, cat[:, :D], dj)
        # linear2 with the gated residual
        w2 = self.W(pre + "linear2.weight")
        y = self.E(M, D)
        branch = self.E(M, D) if (self.save and dmod is not None) else None
        epi2 = dict(epilogue=EPI_GATED_RES, residual=x.d, gate_txt=sl(2), gate_vid=sl(2), gate_bstride=bs, S=Lj, St=0, pre_act_out=branch)
        if q8:
            if catq is not None:                                 # the attention columns: one cast pass
                ops.cast_fp8_scaled(cat[:, :D], catq[:, :D], *self.qsite(site0 + 1))
            if k2:
                self.ff_forward(k2, cate, y, self.W(pre + "linear2.bias"), q8=(self.fp8_in(site0 + 1, cat, catq), site0 + 1, pre + "linear2.weight", None),
                                **epi2)
            else:
                self.mx_gemm(self.fp8_in(site0 + 1, cat, catq), site0 + 1, pre + "linear2.weight", y, self.W(pre + "linear2.bias"), **epi2)
            del catq
        elif k2:
            self.ff_forward(k2, cate, y, self.W(pre + "linear2.bias"), **epi2)
        else:
            ops.gemm(cat, w2, y, self.W(pre + "linear2.bias"), **epi2)
        yv = _Var(y)
        if self.save:
            def bwd_linear2():
                g_ = yv.g
                self.acc(x, g_)
                if dmod is not None:
                    ops.group_colsum(g_, None, y=branch, out2=dsl(2), D=D, S=Lj, St=0, grouped=True, o_bstride=bs, o_segstride=0)
                gge = None
                if k2:                           # proj_out: the extended gradient [gg | dt]; both halves of d(cat) carry dt A
                    gg, ggq, gge = self.gate_mul_q(g_, sl(2), bs, D, Lj, gsite0, ext=fext)
                    self.ff_rank(k2, gge, cat, cate[:, D + M4:])
                else:
                    gg, ggq = self.gate_mul_q(g_, sl(2), bs, D, Lj, gsite0)
                self.colsum(gg, pre + "linear2.bias", D)
                self.dW(gg, cat, self.G(pre + "linear2.weight"))
                dcat = self.E(M, D + M4 + (fext if k1 else 0))       # proj_mlp: d u with its extension columns (bwd_linear1)
                if k2:
                    self.ff_dx(k2, gge, dcat[:, :D], ggq, gsite0, pre + "linear2.weight", rows=(0, D))              # d attn
                elif self.dg:                    # linear2's two column ranges are row slices of its transposed fp8 weight
                    self.dx_gemm(ggq, gsite0, pre + "linear2.weight", dcat[:, :D], rows=(0, D))                     # d attn
                else:
                    ops.gemm(gg, self.P.wt[pre + "linear2.weight"][:D], dcat[:, :D], None)
                # d u = (g W2[:, D:]) * gelu'(u) into the mlp columns (fp8_dgrad: with its quantised copy for linear1's product)
                catv.gq = self.dx_dgelu(gg, ggq, gsite0, gsite0 + 2, pre + "linear2.weight", dcat[:, D:D + M4], u, rows=(D, D + M4), ff=k2, gge=gge)
                catv.g = dcat
                ov.g = dcat[:, :D]
            self.tape.append(bwd_linear2)
        return yv

    def _wt_rows(self, wname, lo, hi):
        key = f"{wname}[{lo}:{hi}]^T"
        if key not in self.P.wt:
            self.P.wt[key] = ops.transpose(self.W(wname)[lo:hi])
        return self.P.wt[key]

    def forward(self, img, txt, vec, txt_valid, freqs):
        m = self.m
        B, Li, D = img.shape
        Lt = txt.shape[1]
        self._Lt = Lt
        self._Lil = Li                                                               # local image rows; the attention's keys: all P shards + valid text
        kv_len = (txt_valid.to(self.dev).to(torch.int32) + Li * self.spP).contiguous()
        rope = None if freqs is None else (freqs[0].to(self.dev, F32).contiguous(), freqs[1].to(self.dev, F32).contiguous())
        self._vec = vec.to(BF16).contiguous()
        sv = self.E(B, D); ops.silu(self._vec, sv)
        svv = _Var(sv)
        self._dsv = torch.zeros(B, D, dtype=F32, device=self.dev) if self.save else None
        iv, tv = _Var(img.to(BF16).reshape(B * Li, D).contiguous()), _Var(txt.to(BF16).reshape(B * Lt, D).contiguous())
        self._in = (iv, tv)
        if self.q8:                 # delayed scaling: the scales of this forward from the amaxes recorded so far (none yet: just in time)
            st = m.fp8_state()
            self.q8s, self.jit = st, not st.seeded
            if st.seeded:
                ops.fp8_scale_update(st.amax, st.history, st.scale)
        for i in range(m.n_double):
            iv, tv = self.double_block(f"double_blocks.{i}.", iv, tv, svv, B, Li, Lt, kv_len, rope, site0=8 * i)
        Lj = Li + Lt
        x = self.E(B, Lj, D)
        x[:, :Li].copy_(iv.d.view(B, Li, D)); x[:, Li:].copy_(tv.d.view(B, Lt, D))          # torch.cat((img, txt), 1) (models.py trunk)
        xv = _Var(x.view(B * Lj, D))
        if self.save:
            def bwd_cat(xv=xv, iv=iv, tv=tv):
                g = xv.g.view(B, Lj, D)
                self.acc(iv, g[:, :Li].reshape(B * Li, D)); self.acc(tv, g[:, Li:].reshape(B * Lt, D))
            self.tape.append(bwd_cat)
        for i in range(m.n_single):
            xv = self.single_block(f"single_blocks.{i}.", xv, svv, B, Li, Lt, kv_len, rope, site0=8 * m.n_double + 2 * i,
                                   gsite0=8 * m.n_double + 3 * i)
        if self.q8:
            self.q8s.seeded = True
        self._out = xv
        self._dims = (B, Lj, D)
        return xv.d.view(B, Lj, D)

    def backward(self, dout):
        B, Lj, D = self._dims
        self._out.g = dout.to(BF16).reshape(B * Lj, D).contiguous()
        if self.dg:                 # delayed scaling of the gradient sites: this backward's scales from the amaxes recorded so far
            st = self.m.fp8_grad_state()
            self.g8s, self.gjit = st, not st.seeded
            if st.seeded:
                ops.fp8_scale_update_fmax(st.amax, st.history, st.scale, self.gfmax)
        while self.tape:
            self.tape.pop()()
        if self.dg:
            self.g8s.seeded = True
        self.lora_scatter()
        iv, tv = self._in
        Li, Lt = iv.d.shape[0] // B, tv.d.shape[0] // B
        if not self.need_dvec:
            return iv.g.view(B, Li, D), tv.g.view(B, Lt, D), None
        dvec = torch.empty(B, D, dtype=F32, device=self.dev)
        ops.silu_bwd(self._dsv, self._vec, dvec)
        return iv.g.view(B, Li, D), tv.g.view(B, Lt, D), dvec.to(BF16)


class HYVideoDiffusionTransformer(HunyuanBlocks):
    """The whole denoiser of hyvideo_t2v/modules/models.py:396-720 under the reference's constructor keys, parameter names and ``forward``
    signature: PatchEmbed, SingleTokenRefiner, TimestepEmbedder / MLPEmbedder modulation vector, the block trunk (HunyuanBlocks), FinalLayer,
    unpatchify.  What TRAINS: the rank-r adapters of ``lora_rank=r`` (the shipped recipe) -- embedders, token refiner and final layer are
    frozen forward code (the final layer with its input gradient); full fine-tuning of the whole model is refused."""

    def __init__(self, args=None, patch_size=(1, 2, 2), in_channels: int = 16, out_channels: Optional[int] = None, hidden_size: int = 3072,
                 heads_num: int = 24, mlp_width_ratio: float = 4.0, mlp_act_type: str = "gelu_tanh", mm_double_blocks_depth: int = 20,
                 mm_single_blocks_depth: int = 40, rope_dim_list=(16, 56, 56), qkv_bias: bool = True, qk_norm: bool = True, qk_norm_type: str = "rms",
                 guidance_embed: bool = False, text_projection: str = "single_refiner", use_attention_mask: bool = True,
                 text_states_dim: Optional[int] = None, text_states_dim_2: Optional[int] = None, fp8: bool = False, lora_rank: int = 0,
                 lora_alpha: float = 1.0, dtype=None, device=None, fp8_amax_history: int = 16, fp8_dgrad=False, lora_target_modules=None,
                 lora_dropout: float = 0.0, **unused):
        if text_projection != "single_refiner" or mlp_act_type != "gelu_tanh" or not qkv_bias or not qk_norm or qk_norm_type != "rms":
            raise NotImplementedError("only the shipped HunyuanVideo-T2V configuration (single_refiner, gelu_tanh, rms qk-norm) is built")
        if sum(rope_dim_list) != hidden_size // heads_num:
            raise ValueError(f"Got {list(rope_dim_list)} but expected positional dim {hidden_size // heads_num}")
        td = text_states_dim if text_states_dim is not None else getattr(args, "text_states_dim", 4096)
        td2 = text_states_dim_2 if text_states_dim_2 is not None else getattr(args, "text_states_dim_2", 768)
        D, M4 = hidden_size, int(hidden_size * mlp_width_ratio)
        pt, ph, pw = patch_size
        oc = in_channels if out_channels is None else out_channels
        before = {"img_in.proj.weight": (D, in_channels, pt, ph, pw), "img_in.proj.bias": (D,),
                  "txt_in.input_embedder.weight": (D, td), "txt_in.input_embedder.bias": (D,),
                  "txt_in.t_embedder.mlp.0.weight": (D, 256), "txt_in.t_embedder.mlp.0.bias": (D,),
                  "txt_in.t_embedder.mlp.2.weight": (D, D), "txt_in.t_embedder.mlp.2.bias": (D,),
                  "txt_in.c_embedder.linear_1.weight": (D, td), "txt_in.c_embedder.linear_1.bias": (D,),
                  "txt_in.c_embedder.linear_2.weight": (D, D), "txt_in.c_embedder.linear_2.bias": (D,)}
        for i in range(2):
            q = f"txt_in.individual_token_refiner.blocks.{i}."
            before.update({q + "norm1.weight": (D,), q + "norm1.bias": (D,), q + "self_attn_qkv.weight": (3 * D, D), q + "self_attn_qkv.bias": (3 * D,),
                           q + "self_attn_proj.weight": (D, D), q + "self_attn_proj.bias": (D,), q + "norm2.weight": (D,), q + "norm2.bias": (D,),
                           q + "mlp.fc1.weight": (M4, D), q + "mlp.fc1.bias": (M4,), q + "mlp.fc2.weight": (D, M4), q + "mlp.fc2.bias": (D,),
                           q + "adaLN_modulation.1.weight": (2 * D, D), q + "adaLN_modulation.1.bias": (2 * D,)})
        before.update({"time_in.mlp.0.weight": (D, 256), "time_in.mlp.0.bias": (D,), "time_in.mlp.2.weight": (D, D), "time_in.mlp.2.bias": (D,),
                       "vector_in.in_layer.weight": (D, td2), "vector_in.in_layer.bias": (D,),
                       "vector_in.out_layer.weight": (D, D), "vector_in.out_layer.bias": (D,)})
        if guidance_embed:
            before.update({"guidance_in.mlp.0.weight": (D, 256), "guidance_in.mlp.0.bias": (D,),
                           "guidance_in.mlp.2.weight": (D, D), "guidance_in.mlp.2.bias": (D,)})
        after = {"final_layer.linear.weight": (pt * ph * pw * oc, D), "final_layer.linear.bias": (pt * ph * pw * oc,),
                 "final_layer.adaLN_modulation.1.weight": (2 * D, D), "final_layer.adaLN_modulation.1.bias": (2 * D,)}
        super().__init__(hidden_size, heads_num, mlp_width_ratio, mm_double_blocks_depth, mm_single_blocks_depth, fp8, lora_rank, lora_alpha,
                         shapes_before=before, shapes_after=after, fp8_amax_history=fp8_amax_history,
                         fp8_dgrad=fp8_dgrad, lora_target_modules=lora_target_modules, lora_dropout=lora_dropout)
        self.patch_size, self.in_channels, self.out_channels, self.guidance_embed = tuple(patch_size), in_channels, oc, guidance_embed
        self.text_states_dim, self.text_states_dim_2 = td, td2

    def enable_training(self):
        raise NotImplementedError("vt355 trains the HunyuanVideo denoiser through its LoRA adapters (lora_rank=r, enable_lora_training()); "
                                  "embedders, token refiner and final layer are frozen forward code")

    # ---- frozen pieces: plain kernel calls, no tape ----
    def _w(self, name):
        return self.flat(self.flat_bf16, name)

    def _lin(self, x, wname, bname, out_dtype=BF16, **epi):
        """x [M, K] bf16 -> x W^T + b; K padded to the GEMM's 64-wide K-tile where a (tiny) input dimension needs it"""
        w, b = self._w(wname), self._w(bname)
        K = w.shape[1]
        if K % 64:
            Kp = (K + 63) // 64 * 64
            xp = torch.zeros(x.shape[0], Kp, dtype=BF16, device=x.device); xp[:, :K] = x
            wp = torch.zeros(w.shape[0], Kp, dtype=BF16, device=x.device); wp[:, :K] = w
            x, w = xp, wp
        y = torch.empty(x.shape[0], w.shape[0], dtype=out_dtype, device=x.device)
        ops.gemm(x.contiguous(), w, y, b, **epi)
        return y

    def _silu(self, x):
        y = torch.empty_like(x)
        ops.silu(x.contiguous(), y)
        return y

    def _tembed(self, t, pre):
        """TimestepEmbedder (embed_layers.py:118-157): cos | sin table (a [B, 256] host-side formula), Linear - SiLU - Linear on the device"""
        import math
        half = 128
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32, device=t.device) / half)
        a = t.float()[:, None] * freqs[None]
        e = torch.cat([torch.cos(a), torch.sin(a)], -1).to(BF16)
        return self._lin(self._silu(self._lin(e, pre + "mlp.0.weight", pre + "mlp.0.bias")), pre + "mlp.2.weight", pre + "mlp.2.bias")

    def _refine_text(self, text_states, t, mask):
        """SingleTokenRefiner (token_refiner.py:163-236) on the device; padding rows attend the valid keys (the reference: key 0) -- they are
        never read by a valid row downstream"""
        B, L, _ = text_states.shape
        D, H = self.hidden_size, self.heads_num
        dev = text_states.device
        temb = self._tembed(t, "txt_in.t_embedder.")
        mf = mask.to(torch.float32).unsqueeze(-1)
        ctx = ((text_states.float() * mf).sum(1) / mf.sum(1)).to(BF16)                 # masked mean over the tokens: [B, text_dim] (host-side reduction)
        ctx = self._lin(self._silu(self._lin(ctx, "txt_in.c_embedder.linear_1.weight", "txt_in.c_embedder.linear_1.bias")),
                        "txt_in.c_embedder.linear_2.weight", "txt_in.c_embedder.linear_2.bias")
        c = torch.empty_like(temb); ops.add_rows(temb, ctx, c)
        sc = self._silu(c)
        x = self._lin(text_states.reshape(B * L, -1).to(BF16), "txt_in.input_embedder.weight", "txt_in.input_embedder.bias")
        klen = mask.sum(1).to(torch.int32).contiguous()
        for i in range(2):
            q = f"txt_in.individual_token_refiner.blocks.{i}."
            gates = self._lin(sc, q + "adaLN_modulation.1.weight", q + "adaLN_modulation.1.bias", out_dtype=F32)        # [B, 2 D]: msa | mlp
            nx = torch.empty_like(x); mean = torch.empty(B * L, dtype=F32, device=dev); rstd = torch.empty_like(mean)
            ops.ln_modulate_fwd(x, nx, self._w(q + "norm1.weight"), self._w(q + "norm1.bias"), None, mean, rstd, D, 1, 0, 1e-6)
            qkv = self._lin(nx, q + "self_attn_qkv.weight", q + "self_attn_qkv.bias").view(B, L, 3 * D)
            o = torch.empty(B, L, D, dtype=BF16, device=dev); lse = torch.empty(B, H, L, dtype=F32, device=dev)
            ops.attn128_fwd(qkv[:, :, :D], qkv[:, :, D:2 * D], qkv[:, :, 2 * D:], o, lse, H, 128 ** -0.5, kv_len=klen)
            x = self._lin(o.view(B * L, D), q + "self_attn_proj.weight", q + "self_attn_proj.bias", epilogue=EPI_GATED_RES, residual=x,
                          gate_txt=gates[:, :D], gate_vid=gates[:, :D], gate_bstride=2 * D, S=L, St=0)
            ops.ln_modulate_fwd(x, nx, self._w(q + "norm2.weight"), self._w(q + "norm2.bias"), None, mean, rstd, D, 1, 0, 1e-6)
            h = self._silu(self._lin(nx, q + "mlp.fc1.weight", q + "mlp.fc1.bias"))
            x = self._lin(h, q + "mlp.fc2.weight", q + "mlp.fc2.bias", epilogue=EPI_GATED_RES, residual=x, gate_txt=gates[:, D:], gate_vid=gates[:, D:],
                          gate_bstride=2 * D, S=L, St=0)
        return x.view(B, L, D)

    def forward(self, x, t, text_states=None, text_mask=None, text_states_2=None, freqs_cos=None, freqs_sin=None, guidance=None,
                return_dict: bool = True):
        """x [B, C, T, H, W], t [B] (0..1000), text_states [B, L, text_dim], text_mask [B, L] (1 = valid), text_states_2 [B, text_dim_2],
        freqs_cos / freqs_sin fp32 [T' H' W', 128] -> [B, C_out, T, H, W] (models.py:592-700)"""
        if not x.is_cuda:
            raise RuntimeError("vt355 HYVideoDiffusionTransformer runs only on an MI355X device (no CPU fallback)")
        B, C, T, Hh, Ww = x.shape
        pt, ph, pw = self.patch_size
        tt, th, tw = T // pt, Hh // ph, Ww // pw
        N, D = tt * th * tw, self.hidden_size
        with torch.no_grad():
            vec = self._tembed(t, "time_in.")
            v2 = self._lin(self._silu(self._lin(text_states_2.to(BF16), "vector_in.in_layer.weight", "vector_in.in_layer.bias")),
                           "vector_in.out_layer.weight", "vector_in.out_layer.bias")
            ops.add_rows(vec, v2, vec)
            if self.guidance_embed:
                if guidance is None:
                    raise ValueError("Didn't get guidance strength for guidance distilled model.")
                ops.add_rows(vec, self._tembed(guidance, "guidance_in."), vec)
            # PatchEmbed: Conv3d with kernel = stride = patch -> a Linear on the gathered patches (channel innermost: the flat layout of conv weights)
            patches = x.to(BF16).reshape(B, C, tt, pt, th, ph, tw, pw).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, N, pt * ph * pw * C)
            lo, Nl = self._sp_rows(N)
            img = self._lin(patches[:, lo:lo + Nl].reshape(B * Nl, -1), "img_in.proj.weight", "img_in.proj.bias").view(B, Nl, D)
            txt = self._refine_text(text_states, t, text_mask)
        tv = text_mask.sum(1)
        freqs = None if freqs_cos is None else (freqs_cos[lo:lo + Nl], freqs_sin[lo:lo + Nl])
        xx = HunyuanBlocks.forward(self, img, txt, vec, tv, freqs)                      # [B, Nl + L, D]; carries the adapters' autograd in LoRA mode
        tokens = Nl != N
        dims = (B, tt, th, tw)
        out = _HYFinal.apply(xx, self, vec, Nl, dims, tokens) if xx.requires_grad else _final_forward(self, xx, vec, Nl, dims, tokens)[0]
        return {"x": out} if return_dict else out

    def patchify(self, x):
        """[B, C_out, T, H, W] -> [B, N, C_out pt ph pw]: the token layout of the final layer's output (the inverse of unpatchify, models.py:702-720);
        under sequence parallelism forward() returns rows ``_sp_rows(N)`` of it"""
        B, oc, T, Hh, Ww = x.shape
        pt, ph, pw = self.patch_size
        tt, th, tw = T // pt, Hh // ph, Ww // pw
        return x.reshape(B, oc, tt, pt, th, ph, tw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, tt * th * tw, oc * pt * ph * pw)


def _final_forward(m: "HYVideoDiffusionTransformer", xx, vec, N, dims, tokens: bool = False):
    """xx [B, N + L, D] -> FinalLayer on the N image rows -> unpatchify; ``tokens``: the rows are one rank's share of the grid, return them as
    tokens [B, N, C_out pt ph pw] (HYVideoDiffusionTransformer.patchify's layout)"""
    B, tt, th, tw = dims
    D = m.hidden_size
    pt, ph, pw = m.patch_size
    oc = m.out_channels
    dev = xx.device
    mod = m._lin(m._silu(vec), "final_layer.adaLN_modulation.1.weight", "final_layer.adaLN_modulation.1.bias", out_dtype=F32)    # shift | scale
    rows = xx[:, :N].reshape(B * N, D).contiguous()
    y = torch.empty_like(rows); mean = torch.empty(B * N, dtype=F32, device=dev); rstd = torch.empty_like(mean)
    ops.ln_modulate_fwd(rows, y, None, None, (mod[:, :D], mod[:, D:], mod[:, :D], mod[:, D:], 2 * D), mean, rstd, D, N, 0, 1e-6)
    tok = m._lin(y, "final_layer.linear.weight", "final_layer.linear.bias")                                                         # [B N, pt ph pw C]
    if tokens:
        return tok.view(B, N, -1), (rows, mean, rstd, mod)
    out = tok.view(B, tt, th, tw, oc, pt, ph, pw).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, oc, tt * pt, th * ph, tw * pw)
    return out, (rows, mean, rstd, mod)


class _HYFinal(torch.autograd.Function):
    """FinalLayer + unpatchify with the gradient w.r.t. the trunk output only (its own weights are frozen)"""

    @staticmethod
    def forward(ctx, xx, m, vec, N, dims, tokens=False):
        out, saved = _final_forward(m, xx, vec, N, dims, tokens)
        ctx.m, ctx.N, ctx.dims, ctx.saved, ctx.shape, ctx.tokens = m, N, dims, saved, xx.shape, tokens
        return out

    @staticmethod
    def backward(ctx, dout):
        m, N, (B, tt, th, tw) = ctx.m, ctx.N, ctx.dims
        rows, mean, rstd, mod = ctx.saved
        D = m.hidden_size
        pt, ph, pw = m.patch_size
        oc = m.out_channels
        if ctx.tokens:
            dtok = dout.to(BF16).reshape(B * N, oc * pt * ph * pw)
        else:
            dtok = dout.to(BF16).reshape(B, oc, tt, pt, th, ph, tw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * N, oc * pt * ph * pw)
        w = m._w("final_layer.linear.weight")                         # [n_out, D]
        n_out = w.shape[0]
        Kp = (n_out + 63) // 64 * 64
        gp = torch.zeros(B * N, Kp, dtype=BF16, device=dout.device); gp[:, :n_out] = dtok
        wt = torch.zeros(D, Kp, dtype=BF16, device=dout.device); wt[:, :n_out] = w.t()
        dy = torch.empty(B * N, D, dtype=BF16, device=dout.device)
        ops.gemm(gp, wt, dy, None)
        dx = torch.empty_like(dy)
        ops.ln_modulate_bwd(dy, rows, mean, rstd, None, (mod[:, D:], mod[:, D:], 2 * D), None, dx, D, N, 0)
        dxx = torch.zeros(ctx.shape, dtype=BF16, device=dout.device)
        dxx[:, :N] = dx.view(B, N, D)
        return dxx, None, None, None, None, None


def rope_tables(sizes, rope_dim_list=(16, 56, 56), theta: float = 256.0):
    """get_nd_rotary_pos_embed(rope_dim_list, sizes, theta, use_real=True) of modules/posemb_layers.py:191-258 as inference.py:470-495 calls it
    (rope_sizes = latent size // patch size, theta = args.rope_theta = 256): (cos, sin) fp32 [prod(sizes), sum(rope_dim_list)], every
    frequency repeated for its (2i, 2i+1) pair; axis i contributes rope_dim_list[i] columns from its own coordinate."""
    grids = torch.meshgrid(*[torch.arange(n, dtype=torch.float32) for n in sizes], indexing="ij")
    cos, sin = [], []
    for dim, gr in zip(rope_dim_list, grids):
        freqs = 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim))
        a = torch.outer(gr.reshape(-1), freqs)
        cos.append(a.cos().repeat_interleave(2, dim=1)); sin.append(a.sin().repeat_interleave(2, dim=1))
    return torch.cat(cos, 1), torch.cat(sin, 1)


class HunyuanVideoFlow(torch.nn.Module):
    """training_step of HunyuanVideoWorkFlow (hyvideo_t2v/hunyuanvideo.py:883-971) around vt355's denoiser: sigma drawn uniformly from the
    scheduler's table (flow_weighting_scheme "none"), timesteps = (sigma * 1000).long(), x_t = (1 - sigma) x0 + sigma eps, target eps - x0, mean
    squared error.  Batches come pre-encoded -- {"latents" [B, C, T, H, W], "prompt_embeds" [B, L, text_dim], "prompt_attention_mask" [B, L],
    "pooled_prompt_embeds" [B, text_dim_2]} -- the causal VAE and the LLM / CLIP text encoders of that workflow are frozen neighbours outside
    this path.  The scheduler's sigma table is linspace(1, 1/N, N) with an optional shift (the checkpoint's scheduler config is not available
    offline: flow_shift is a constructor argument)."""

    def __init__(self, denoiser_config=None, model: Optional[HYVideoDiffusionTransformer] = None, num_train_timesteps: int = 1000,
                 flow_shift: float = 1.0, learning_rate: float = 1e-5, rope_theta: float = 256.0, **unused):
        super().__init__()
        if model is None:
            from .config import instantiate_from_config
            model = instantiate_from_config(denoiser_config)
        self.model, self.learning_rate, self.rope_theta = model, learning_rate, rope_theta
        s = torch.linspace(1.0, 1.0 / num_train_timesteps, num_train_timesteps)
        self.register_buffer("sigmas", flow_shift * s / (1.0 + (flow_shift - 1.0) * s), persistent=False)
        self._rope = {}

    def configure_optimizers(self, gradient_clip_val=None, gradient_clip_algorithm="norm"):
        """gradient_clip_val / gradient_clip_algorithm: Lightning's trainer options (config.trainer_options reads them from a recipe)"""
        from .optim import FusedAdamW
        ts = self.model.enable_lora_training()
        return FusedAdamW(ts.params, lr=self.learning_rate, fullft_state=ts, gradient_clip_val=gradient_clip_val,
                          gradient_clip_algorithm=gradient_clip_algorithm)

    def loss_from(self, x0, prompt_embeds, mask, pooled, sigma, noise, guidance=None):
        dev = x0.device
        B, C, T, Hh, Ww = x0.shape
        pt, ph, pw = self.model.patch_size
        key = (T // pt, Hh // ph, Ww // pw)
        if key not in self._rope:
            cos, sin = rope_tables(key, theta=self.rope_theta)
            self._rope[key] = (cos.to(dev), sin.to(dev))
        s5 = sigma.view(-1, 1, 1, 1, 1).float()
        xt = ((1.0 - s5) * x0.float() + s5 * noise.float()).to(BF16)
        t = (sigma * 1000.0).long()
        out = self.model(xt, t, text_states=prompt_embeds, text_mask=mask, text_states_2=pooled, freqs_cos=self._rope[key][0],
                         freqs_sin=self._rope[key][1], guidance=guidance, return_dict=False)
        if self.model.sp_group is not None:
            # sequence parallel: the model returned this rank's rows of the prediction as tokens; the mean squared error over ITS rows (the
            # mean over the group's ranks is the loss of the step; a reducer that averages gradients over all ranks does the rest)
            lo, Nl = self.model._sp_rows(out.shape[1] * torch.distributed.get_world_size(self.model.sp_group))
            return _FlowLoss.apply(out, self.model.patchify(x0.float())[:, lo:lo + Nl].contiguous(), self.model.patchify(noise.float())[:, lo:lo + Nl].contiguous())
        return _FlowLoss.apply(out, x0.float(), noise.float())

    def training_step(self, batch, batch_idx=0):
        x0 = batch["latents"]
        B = x0.shape[0]
        idx = (torch.rand(B, device=x0.device) * self.sigmas.numel()).long().clamp_(max=self.sigmas.numel() - 1)
        noise = torch.randn_like(x0, dtype=torch.float32)
        group = self.model.sp_group
        if group is not None:                       # one sample, one sigma, one noise for the ranks that share its rows (the batch is the caller's)
            src = torch.distributed.get_global_rank(group, 0)
            torch.distributed.broadcast(idx, src, group=group); torch.distributed.broadcast(noise, src, group=group)
        sigma = self.sigmas.to(x0.device)[idx]
        guidance = torch.full((B,), 1000.0, device=x0.device) if self.model.guidance_embed else None
        pinned = self.model.lora_dropout_seed
        if group is not None and pinned is None and self.model.lora_dropout > 0 and self.model.training:
            # lora_dropout: the ranks that share a sample's rows share its masks -- group rank 0 draws the step's seed (engine's rule)
            drawn = lora_dropout_seed(self.model)[1] if torch.distributed.get_rank(group) == 0 else 0
            seed = torch.tensor([drawn], dtype=torch.int64, device=x0.device)
            torch.distributed.broadcast(seed, src, group=group)
            self.model.lora_dropout_seed = int(seed.item())
        try:
            return self.loss_from(x0, batch["prompt_embeds"], batch["prompt_attention_mask"], batch["pooled_prompt_embeds"], sigma, noise, guidance)
        finally:
            self.model.lora_dropout_seed = pinned


class _FlowLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, x0, noise):
        loss, dpred = flow_matching_loss(out.contiguous().view(out.shape[0], -1), x0.reshape(out.shape[0], -1), noise.reshape(out.shape[0], -1))
        ctx.save_for_backward(dpred)
        ctx.shape = out.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return (dpred.float() * g).to(BF16).view(ctx.shape), None, None


def flow_matching_loss(pred, x0, noise):
    """mean_b mean (pred - (noise - x0))^2 (hunyuanvideo.py:963-970, weights 1); pred bf16, x0 / noise fp32 -> (loss fp32 [1], dpred bf16)"""
    target = torch.empty_like(x0)
    torch.sub(noise, x0, out=target)
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred)
    ops.mse_loss(pred.contiguous(), target, loss, dpred)
    return loss, dpred
