"""TEST INFRASTRUCTURE: the CogVideoX sampler restated in fp64 numpy -- the Philox normals of include/vt355.h's noise convention (on
oracle/philox.philox4x32_10), the timestep lists and host coefficients of diffusers' CogVideoXDPMScheduler, one guidance + DPM-Solver++
step, and the whole loop around a `denoise(x, t)` callable.  Written from the rules in the header and the scheduler's documentation, not
from the product's Python: vt355 does not import this file and this file does not import vt355.

Pinned by tests/golden/dpm_sampler.npz (the in-tree twin VPSDEDPMPP2MSampler, cogvideo_sat/sgm/modules/diffusionmodules/sampling.py:762-869).
MUTANTS lists the wrong loops a test's inputs have to tell from the right one (tests/test_sampler_cpu.py prints the separations)."""
import math

import numpy as np

from philox import philox4x32_10

BF16_STEP = 2.0 ** -7          # one step of the bf16 grid relative to the value (8 significant bits)
# bars of the GPU step / loop tests, shared with the mutant-separation test
X0_RTOL, X0_ATOL = 1e-5, 1e-5
# latents: one bf16 step, plus the x0 bar's absolute term -- x' is a three-term fp32 sum of the same magnitudes as x0's two-term one, so near a
# cancellation its fp32 error is the one the x0 bar already allows
LAT_RTOL, LAT_ATOL = BF16_STEP, 1e-5


# ------------------------------------------------------------------ noise convention
def philox_normal(n, B, seed, stream):
    """fp64 [B, n]: element e of sample b from Philox4x32-10(key = seed + b, counter = (stream << 40) + e // 4), Box-Muller on the word
    pairs (0, 1) and (2, 3) with u1 = ((w >> 8) + 1) 2^-24, u2 = (w' >> 8) 2^-24"""
    quads = (n + 3) // 4
    assert 0 <= stream < (1 << 24) and quads <= (1 << 40)
    c64 = (np.uint64(stream) << np.uint64(40)) + np.arange(quads, dtype=np.uint64)
    ctr = np.zeros((quads, 4), dtype=np.uint32)
    ctr[:, 0] = (c64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (c64 >> np.uint64(32)).astype(np.uint32)
    out = np.empty((B, quads * 4), dtype=np.float64)
    for b in range(B):
        k = (int(seed) + b) & 0xFFFFFFFFFFFFFFFF
        w = philox4x32_10(ctr, np.array([k & 0xFFFFFFFF, k >> 32], dtype=np.uint32)).astype(np.uint64)
        for p in range(2):
            u1 = ((w[:, 2 * p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
            u2 = (w[:, 2 * p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
            rad = np.sqrt(-2.0 * np.log(u1))
            out[b, 2 * p::4] = rad * np.cos(2.0 * np.pi * u2)
            out[b, 2 * p + 1::4] = rad * np.sin(2.0 * np.pi * u2)
    return out[:, :n]


# ------------------------------------------------------------------ schedule
def timesteps(N, n, spacing, steps_offset=0):
    if spacing == "leading":
        return [int(round(i * (N // n))) + steps_offset for i in range(n)][::-1]
    if spacing == "linspace":
        return [int(v) for v in np.linspace(0, N - 1, n).round()[::-1]]
    if spacing == "trailing":
        return [int(v) - 1 for v in np.round(np.arange(N, 0, -N / n))]
    raise ValueError(spacing)


def _lam(a):
    with np.errstate(divide="ignore"):
        return np.log(np.sqrt(np.float64(a) / (1.0 - np.float64(a))))


def coefficients(a_t, a_prev, a_back=None):
    """dict(h, m1, m2, m_noise[, r, m3, m4]) of one step from the cumulative alphas, fp64; infinities where the rules give them"""
    a_t, a_prev = np.float64(a_t), np.float64(a_prev)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        h = _lam(a_prev) - _lam(a_t)
        c = {"h": float(h), "m1": float(np.sqrt((1 - a_prev) / (1 - a_t)) * np.exp(-h)), "m2": float(np.expm1(-2 * h) * np.sqrt(a_prev)),
             "m_noise": float(np.sqrt(1 - a_prev) * np.sqrt(1 - np.exp(-2 * h)))}
        if a_back is not None:
            r = (_lam(a_t) - _lam(a_back)) / h
            c.update(r=float(r), m3=float(1 + 1 / (2 * r)), m4=float(1 / (2 * r)))
    return c


def step_plan(abar, ts, i, N, final_abar, have_old, mutant=None):
    """the scalars of step i of the list ts: dict(sa, sb, m1, m2, m3, m4, m_noise, second_order)"""
    n, t = len(ts), ts[i]
    prev_t = t - N // n
    if mutant == "prev_from_list":
        prev_t = ts[i + 1] if i + 1 < n else -1
    a_prev = abar[prev_t] if prev_t >= 0 else final_abar
    second = have_old and prev_t >= 0
    if mutant == "last_second_order":
        second = have_old
    back = None
    if second:
        back = ts[i - 1]
        if mutant == "back_is_next":
            back = ts[i + 1] if i + 1 < n else 0
    c = coefficients(abar[t], a_prev, abar[back] if second else None)
    if second and mutant == "m3_m4_swapped":
        c["m3"], c["m4"] = c["m4"], c["m3"]
    c.update(sa=math.sqrt(abar[t]), sb=math.sqrt(1 - abar[t]), second_order=second)
    return c


# ------------------------------------------------------------------ one step, the loop
def step(v, x, x0_old, eps, c, g=None):
    """(x', x0) in fp64.  v [2B, ...] = (uncond, cond) with a guidance scale g, else [B, ...]; c from step_plan"""
    v = np.asarray(v, dtype=np.float64); x = np.asarray(x, dtype=np.float64)
    if g is not None:
        B = x.shape[0]
        v = v[:B] + g * (v[B:] - v[:B])
    x0 = c["sa"] * x - c["sb"] * v
    with np.errstate(invalid="ignore", over="ignore"):
        d = c["m3"] * x0 - c["m4"] * np.asarray(x0_old, dtype=np.float64) if c["second_order"] else x0
        xn = c["m1"] * x - c["m2"] * d
    if c["m_noise"] != 0.0:
        xn = xn + c["m_noise"] * np.asarray(eps, dtype=np.float64)
    return xn, x0


def dynamic_cfg(g, n, t):
    return 1 + g * ((1 - math.cos(math.pi * ((n - t) / n) ** 5.0)) / 2)


def loop(x, denoise, abar, ts, N, final_abar, seed, g=None, dynamic=False, mutant=None, noise=None):
    """the sampling loop in fp64: returns the list of latents after every step.  denoise(x, t) -> v ([2B, ...] when g is given).
    Step i's noise is Philox stream i + 1 of `seed` (or noise[i] when a recorded list is given)."""
    x = np.asarray(x, dtype=np.float64)
    B, per = x.shape[0], int(np.prod(x.shape[1:]))
    old, out = None, []
    for i, t in enumerate(ts):
        v = np.asarray(denoise(x, t), dtype=np.float64)
        if g is not None and mutant == "halves_swapped":
            v = np.concatenate([v[B:], v[:B]])
        c = step_plan(abar, ts, i, N, final_abar, old is not None, mutant)
        if noise is not None:
            eps = noise[i]
        else:
            eps = philox_normal(per, B, seed, i if mutant == "stream_i" else i + 1)
            if mutant == "one_key":
                eps = np.repeat(eps[:1], B, axis=0)
            eps = eps.reshape(x.shape)
        gi = None if g is None else (dynamic_cfg(g, len(ts), t) if dynamic else g)
        x, old = step(v, x, old, eps, c, gi)
        out.append(x)
    return out


MUTANTS = ["halves_swapped",        # cond / uncond halves of the model output swapped
           "back_is_next",          # timestep_back taken as the next list entry, not the previous one
           "prev_from_list",        # prev_timestep taken from the list, not t - N // n
           "m3_m4_swapped",
           "last_second_order",     # the prev_timestep < 0 rule dropped: the last step second order (m3 = m4 = inf)
           "stream_i",              # step i drawing stream i (the initial latents' stream at i = 0), not stream i + 1
           "one_key"]               # key `seed` for every sample, not seed + b


def linear_denoiser(B, guided=True):
    """a stub v(x, t), linear in x, with different uncond / cond branches and a t-dependent offset"""
    def f(x, t):
        s = math.sin(t / 100.0)
        vu = 0.3 * x + 0.1 * s
        vc = -0.5 * x + 0.2 + 0.05 * s
        return np.concatenate([vu, vc]) if guided else vc
    return f


def separation(a, b):
    """max over elements of |a - b| in units of the latent bar at b; inf when a is not finite"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.isfinite(a).all():
        return math.inf
    return float(np.max(np.abs(a - b) / (LAT_ATOL + LAT_RTOL * np.abs(b))))
