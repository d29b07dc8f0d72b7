"""Plain fp64 restatements of the memory-bound glue kernels (csrc/elementwise.hip, the GEGLU / row-map / loss / q-sample sections of
csrc/unet_ops.hip, the gated-GELU and residual-cast kernels of csrc/t5.hip), written from the reference semantics the kernels' own
comments cite, and SWEEPS: the grid cap of every kernel that walks its data with a capped grid-stride loop, next to the shape at which
tests/test_glue_kernels_gpu.py sends a thread round that loop a second time.

Every function takes torch tensors on any device and computes in the dtype it is given: fp64 inputs give the reference, the same call on
fp32 inputs gives the "fp32 evaluation" whose distance from fp64 prices a transcendental kernel's function error.  Nothing here calls
torch.nn.functional: tests/test_glue_ref_cpu.py checks these restatements AGAINST the PyTorch calls they restate."""
import math

import torch

SQRT1_2 = 0.7071067811865476
SQRT_2_PI = 0.7978845608028654


# ------------------------------------------------------------------ one rounding
def round_once_bf16(x64):
    """fp64 -> bf16 in ONE round-to-nearest-even step, on the bits (x.to(bfloat16) would round through fp32 first)"""
    b = x64.view(torch.int64)
    drop = 52 - 7                                  # fp64 keeps 52 fraction bits, bf16 7; both exponents cover the values used here
    low = b & ((1 << drop) - 1)
    half = 1 << (drop - 1)
    up = (low > half) | ((low == half) & (((b >> drop) & 1) == 1))
    r = ((b >> drop) + up.to(torch.int64)) << drop
    return r.view(torch.float64)


# ------------------------------------------------------------------ activations
def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x * SQRT1_2))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x * SQRT1_2)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + torch.tanh(SQRT_2_PI * (x + 0.044715 * x * x * x)))


def geglu_fwd(h):
    """h [M, 2F] = (a | gate) -> a * gelu_erf(gate)   (GEGLU of the UNet's FeedForward)"""
    a, g = h.chunk(2, dim=-1)
    return a * gelu_erf(g)


def geglu_bwd(dy, h):
    """-> dh [M, 2F] = (dy * gelu(gate) | dy * a * gelu'(gate))"""
    a, g = h.chunk(2, dim=-1)
    return torch.cat([dy * gelu_erf(g), dy * a * gelu_erf_grad(g)], dim=-1)


def gated_gelu(u):
    """u [M, 2F] = (x Wi0^T | x Wi1^T) -> gelu_new(first half) * second half   (T5DenseGatedActDense)"""
    a, b = u.chunk(2, dim=-1)
    return gelu_tanh(a) * b


# ------------------------------------------------------------------ row maps (rows of C elements)
def row_map(src, mode, nb, d1, d2):
    """src: 2-d rows.  0: [nb, d1, d2] -> [nb, d2, d1]; 1: nearest x2 of [nb, d1, d2]; 2: zero insertion, same shapes;
    3: sum of the 2x2 blocks, src [nb, 2 d1, 2 d2] -> [nb, d1, d2]"""
    C = src.shape[1]
    if mode == 0:
        out = torch.empty(nb, d2, d1, C, dtype=src.dtype, device=src.device)
        s = src.reshape(nb, d1, d2, C)
        for a1 in range(d1):
            out[:, :, a1] = s[:, a1]
        return out.reshape(-1, C)
    if mode in (1, 2):
        s = src.reshape(nb, d1, d2, C)
        out = torch.zeros(nb, 2 * d1, 2 * d2, C, dtype=src.dtype, device=src.device)
        for dh in range(2):
            for dw in range(2):
                if mode == 1 or (dh == 0 and dw == 0):
                    out[:, dh::2, dw::2] = s
        return out.reshape(-1, C)
    if mode == 3:
        s = src.reshape(nb, 2 * d1, 2 * d2, C)
        return (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]).reshape(-1, C)
    raise ValueError(mode)


def row_map_terms(src, mode, nb, d1, d2):
    """sum of |terms| of one output element (the magnitude a one-ulp bar is taken on)"""
    return row_map(src.abs(), mode, nb, d1, d2)


def gate_rows(M, S, St):
    """(sample index, is-text) of each of M rows: row m belongs to sample m // S, and is a text row when m % S < St"""
    m = torch.arange(M)
    return m // S, (m % S) < St


# ------------------------------------------------------------------ patchify: [B, F, C, H, W] <-> tokens (t h w) x columns (c p q)
def patchify(img, P):
    B, F, C, H, W = img.shape
    hh, ww = H // P, W // P
    tok = torch.empty(B * F * hh * ww, C * P * P, dtype=img.dtype, device=img.device)
    t4 = tok.view(B, F, hh, ww, C, P, P)
    for p in range(P):
        for q in range(P):
            t4[..., p, q] = img[:, :, :, p::P, q::P].permute(0, 1, 3, 4, 2)
    return tok


def unpatchify(tok, B, F, C, H, W, P):
    hh, ww = H // P, W // P
    img = torch.empty(B, F, C, H, W, dtype=tok.dtype, device=tok.device)
    t4 = tok.reshape(B, F, hh, ww, C, P, P)
    for p in range(P):
        for q in range(P):
            img[:, :, :, p::P, q::P] = t4[..., p, q].permute(0, 1, 4, 2, 3)
    return img


# ------------------------------------------------------------------ sinusoidal timestep embedding
def timestep_embedding(t, D, flip=True, freq_shift=0.0, max_period=10000.0, dtype=torch.float64):
    """diffusers' get_timestep_embedding(scale = 1): freq_k = exp(-ln(max_period) * k / (D/2 - freq_shift)), out = [sin | cos], halves
    swapped when flip (flip_sin_to_cos).  dtype = float32 evaluates the same formula in fp32, operation by operation."""
    half = D // 2
    k = torch.arange(half, dtype=dtype)
    expo = torch.tensor(-math.log(max_period), dtype=dtype) * k / (torch.tensor(float(half), dtype=dtype) - torch.tensor(freq_shift, dtype=dtype))
    arg = t.to(dtype)[:, None] * torch.exp(expo)[None, :]
    s, c = torch.sin(arg), torch.cos(arg)
    return torch.cat([c, s], dim=-1) if flip else torch.cat([s, c], dim=-1)


# ------------------------------------------------------------------ forward process and losses
def _per_sample(v, x):
    return v.to(x.dtype).view(-1, *([1] * (x.dim() - 1)))


def add_noise(x0, noise, sa, sb):
    """sqrt(abar_t) x0 + sqrt(1 - abar_t) eps, per sample"""
    return _per_sample(sa, x0) * x0 + _per_sample(sb, x0) * noise


def q_sample(x0, noise, sa, sb, scale=None):
    """ddpm3d.py q_sample with the optional per-sample scale_arr[t] on x0"""
    a = _per_sample(sa, x0) * (_per_sample(scale, x0) if scale is not None else 1.0)
    return a * x0 + _per_sample(sb, x0) * noise


def diffusion_loss(vpred, noisy, x0, sa, sb, w):
    """CogVideoX v-prediction loss: x0_hat = sa x_t - sb v; mean_b mean_i w_b (x0_hat - x0)^2"""
    pred = _per_sample(sa, x0) * noisy - _per_sample(sb, x0) * vpred
    return (_per_sample(w, x0) * (pred - x0) ** 2).flatten(1).mean(1).mean()


def diffusion_loss_grad(vpred, noisy, x0, sa, sb, w):
    """(d loss / d vpred, sum of |terms| of the short expression behind each element)"""
    n = x0.numel()
    pred_terms = (_per_sample(sa, x0) * noisy).abs() + (_per_sample(sb, x0) * vpred).abs() + x0.abs()
    pred = _per_sample(sa, x0) * noisy - _per_sample(sb, x0) * vpred
    k = 2.0 / n * _per_sample(w, x0) * (-_per_sample(sb, x0))
    return k * (pred - x0), k.abs() * pred_terms


def mse_loss(pred, target):
    return ((pred - target) ** 2).flatten(1).mean(1).mean()


def mse_loss_grad(pred, target):
    k = 2.0 / pred.numel()
    return k * (pred - target), k * (pred.abs() + target.abs())


def _normal_cdf_approx(x):
    return 0.5 * (1.0 + torch.tanh(SQRT_2_PI * (x + 0.044715 * x ** 3)))


def opensora_loss(out, x0, noise, coef):
    """IDDPM p_losses (EPSILON mean, LEARNED_RANGE variance, MSE): out [B, 2C, ...] = (eps_hat | v); coef fp64 [B, 8] = sqrt_ac, sqrt_1mac,
    coef1, coef2, min_log, max_log, (t == 0), unused.  Returns (loss, mse, vb).  The mean prediction is detached inside vb and takes the
    RAW eps_hat where x0 is expected (the reference's quirk)."""
    C = x0.shape[1]
    cf = [_per_sample(coef[:, j], x0) for j in range(7)]
    eps_hat, v = out[:, :C], out[:, C:]
    x_t = cf[0] * x0 + cf[1] * noise
    frac = (v + 1.0) / 2.0
    lv = frac * cf[5] + (1.0 - frac) * cf[4]
    mean_p = cf[2] * eps_hat.detach() + cf[3] * x_t
    mean_t = cf[2] * x0 + cf[3] * x_t
    kl = 0.5 * (-1.0 + lv - cf[4] + torch.exp(cf[4] - lv) + (mean_t - mean_p) ** 2 * torch.exp(-lv))
    centered = x0 - mean_p
    inv_std = torch.exp(-0.5 * lv)
    cdf_p = _normal_cdf_approx(inv_std * (centered + 1.0 / 255.0))
    cdf_m = _normal_cdf_approx(inv_std * (centered - 1.0 / 255.0))
    ll = torch.where(x0 < -0.999, torch.log(cdf_p.clamp(min=1e-12)),
                     torch.where(x0 > 0.999, torch.log((1.0 - cdf_m).clamp(min=1e-12)), torch.log((cdf_p - cdf_m).clamp(min=1e-12))))
    vb = torch.where(coef[:, 6] != 0, (-ll).flatten(1).mean(1), kl.flatten(1).mean(1)) / math.log(2.0)
    mse = ((noise - eps_hat) ** 2).flatten(1).mean(1)
    return (mse + vb).mean(), mse.mean(), vb.mean()


# ------------------------------------------------------------------ AdamW (torch.optim.AdamW, decoupled decay before the step)
def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    """-> (p_new, m_new, v_new, update) with update = p * (1 - lr wd) - p_new = lr / bc1 * m_new / (sqrt(v_new) / sqrt(bc2) + eps)"""
    g = g * grad_scale
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    upd = (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p * (1.0 - lr * wd) - upd, m, v, upd


# ------------------------------------------------------------------ capped grids
def _chunked(M, W):
    return {"items": M * (W // 8), "per_row": W // 8}


def _flat(B, per):
    return {"items": B * per, "per_row": per}


# entry point, cap in workgroups of 256 threads, where the cap was read, loop unit (elements per work item), the wrap shape of the GPU
# test, its work items and the divisor of the loop's index split (chunks per row / elements per sample), and the sweeps it may take.
_WIDE = dict(M=16400, F=2056)
SWEEPS = [
    dict(entry="vt_geglu_fwd", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=_WIDE, **_chunked(16400, 2056)),
    dict(entry="vt_geglu_bwd", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=_WIDE, **_chunked(16400, 2056)),
    dict(entry="vt_add_rows_bf16", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=_WIDE, **_chunked(16400, 2056)),
    dict(entry="vt_dropout_bf16", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=_WIDE, **_chunked(16400, 2056)),
    dict(entry="vt_gated_gelu_bf16", cap=16384, where="videotuna-dev_amd/csrc/t5.hip:68", unit=8, shape=_WIDE, **_chunked(16400, 2056)),
    dict(entry="vt_residual_cast_bf16", cap=16384, where="videotuna-dev_amd/csrc/t5.hip:100", unit=8, shape=_WIDE, **_chunked(16400, 2056)),
    dict(entry="vt_row_map_bf16 mode 0", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=dict(nb=2, d1=5, d2=1640, C=2056),
         **_chunked(2 * 5 * 1640, 2056)),
    dict(entry="vt_row_map_bf16 mode 1", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=dict(nb=2, d1=41, d2=50, C=2056),
         **_chunked(2 * 4 * 41 * 50, 2056)),
    dict(entry="vt_row_map_bf16 mode 2", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=dict(nb=2, d1=41, d2=50, C=2056),
         **_chunked(2 * 4 * 41 * 50, 2056)),
    # work items are OUTPUT rows: nb = 1 (4 100 output rows, 2 103 300 chunks) would stay inside the first sweep, so the wrap case is nb = 2
    dict(entry="vt_row_map_bf16 mode 3", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=8, shape=dict(nb=2, d1=82, d2=50, C=4104),
         **_chunked(2 * 82 * 50, 4104)),
    dict(entry="vt_gate_mul", cap=8192, where="videotuna-dev_amd/csrc/elementwise.hip:35", unit=8, shape=dict(B=4, S=2048, D=2056, St=77), **_chunked(4 * 2048, 2056)),
    dict(entry="vt_patchify", cap=8192, where="videotuna-dev_amd/csrc/elementwise.hip:107", unit=1, shape=dict(B=2, F=3, C=16, H=132, W=168, P=2),
         **_flat(2 * 3 * 16 * 132, 168)),
    dict(entry="vt_unpatchify", cap=8192, where="videotuna-dev_amd/csrc/elementwise.hip:114", unit=1, shape=dict(B=2, F=3, C=16, H=132, W=168, P=2),
         **_flat(2 * 3 * 16 * 132, 168)),
    dict(entry="vt_cast_f32_bf16", cap=8192, where="videotuna-dev_amd/csrc/elementwise.hip:59", unit=1, shape=dict(n=2 * 2097152 + 77), **_flat(1, 2 * 2097152 + 77)),
    dict(entry="vt_add_noise", cap=4096, where="videotuna-dev_amd/csrc/elementwise.hip:132", unit=1, shape=dict(B=3, per=350003), **_flat(3, 350003)),
    dict(entry="vt_q_sample", cap=16384, where="videotuna-dev_amd/csrc/unet_ops.hip:219", unit=1, shape=dict(B=3, per=1400003), **_flat(3, 1400003)),
    dict(entry="vt_diffusion_loss", cap=512, where="videotuna-dev_amd/csrc/elementwise.hip:138", unit=1, shape=dict(B=3, per=100003), **_flat(3, 100003)),
    dict(entry="vt_diffusion_loss_bwd", cap=512, where="videotuna-dev_amd/csrc/elementwise.hip:138", unit=1, shape=dict(B=3, per=100003), **_flat(3, 100003)),
    # 3 x 524 313 is 75 elements more than three sweeps: the fourth sweep is one partly filled workgroup
    dict(entry="vt_mse_loss", cap=2048, where="videotuna-dev_amd/csrc/unet_ops.hip:407", unit=1, shape=dict(B=3, per=524313), max_sweeps=4, **_flat(3, 524313)),
    dict(entry="vt_opensora_loss", cap=1024, where="videotuna-dev_amd/csrc/unet_ops.hip:489", unit=1, shape=dict(B=2, C=4, per_c=40003), **_flat(2, 4 * 40003)),
    dict(entry="vt_adamw", cap=16384, where="videotuna-dev_amd/csrc/elementwise.hip:228", unit=1, shape=dict(n=4194304 + 4099), **_flat(1, 4194304 + 4099)),
]


def sweep(entry):
    rows = [r for r in SWEEPS if r["entry"] == entry]
    assert len(rows) == 1, entry
    return rows[0]
