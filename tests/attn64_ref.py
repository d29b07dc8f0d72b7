"""Inputs, fp64 references and a CPU restatement of the lazy-maximum policy for the head_dim-64 attention kernels
(csrc/attn_fwd.hip: attn_fwd_hd64_kernel<PRESCALED, BIAS>, attn_fwd_hd64_m16_kernel; csrc/attn_bwd.hip).

  * qkv_case: randn and the three ill-conditioned key families of conditioning_ref at head_dim 64, with the bf16 prescaling of q that the
    training path applies (q * scale * log2e re-rounded; the reference is fed exactly what the kernel sees).
  * reference: conditioning_ref.dense_attention64 in fp64 -> o, lse2, d qkv.  Computed once per case and shared.
  * lazy_policy64: the hd64 forward's policy, which is not attn128's.  The reference starts at 0 (the accumulators of S^T start at -m_ref);
    tile 0 moves it by the tile maximum (up or down); a later tile moves it by max(rise, 0), and only when some lane group of some row of the
    wave sees a rise of more than 8 log2 units.  The lane groups exchange their maxima only inside that branch.
  * CHAIN_CASES / chain_plan_expected: the smallest backward shapes at which a dQ hand-off chain exists, with the plan each must get, written
    down by hand from the kernel's scheduling rules (not computed by a copy of the library's launch code).
Pure torch, no GPU: the CPU and the GPU tests draw identical tensors from a seed."""
import functools

import torch

from conditioning_ref import LOG2E, SOFTMAX_CASES, dense_attention64, rb, saturated_rows, scale_keys

HD = 64
SC2 = LOG2E / 8.0                     # softmax_scale * log2(e) at head_dim 64
EXTREME_CASES = ("all_low", "early_giant")      # see qkv_case; the only inputs here with saturated rows, and meant to have them
CASES = ("randn",) + SOFTMAX_CASES + EXTREME_CASES
FK = 64                               # keys per forward tile
WAVE_ROWS = 32                        # query rows per forward wave
LAZY_THR = 8.0                        # attn_fwd.hip: LAZY_THR
_NEG = -1.0e30                        # attn_fwd.hip: NEG_BIG, the score of a key past S in the ragged last tile

# Sizes of the GPU tests (tests/test_attn64_gpu.py); the CPU tests check the reference on every one of them.
FWD_EDGE_S = (1, 31, 63, 64, 65, 127, 128, 129, 193, 257)           # (B, H) = (2, 3): below one key tile, at and just past 64 / 128 / 256
FWD_LATE = ((1, 2, 333), (2, 3, 193))                               # (B, H, S) of the late-maximum cases
# late_spike around a ragged last tile.  S = 65, 129: the last tile holds ONE key, the x 12 key S - 3 is the last but one of the full tile in
# front of it (at S = 65 that is tile 0: no rescale at all, the 63 masked scores must move nothing).  S = 67, 131: the x 12 key is the first
# of a three-key ragged tile, which therefore rescales
FWD_SPIKE_S = (65, 67, 129, 131)
BWD_EDGE_S = (1, 31, 64, 65, 255, 256, 257, 320, 513)               # (B, H) = (2, 2): 256-key blocks, 64-query steps, 32-key waves
BWD_LATE = ((1, 2, 333), (1, 2, 513))


def key_groups(variant):
    """lane group of each of the 64 keys of a tile: which lanes of a query column hold the key's score.
      m32  attn_fwd_hd64_kernel: register i of lane half h holds key 32 kt2 + (i & 3) + 8 (i >> 2) + 4 h  ->  half = (key % 8) // 4
      m16  attn_fwd_hd64_m16_kernel: register i of lane group g holds key 16 kt + 4 g + i                  ->  group = (key % 16) // 4"""
    key = torch.arange(FK)
    if variant == "m32":
        return (key % 8) // 4, 2
    if variant == "m16":
        return (key % 16) // 4, 4
    raise KeyError(variant)


@functools.lru_cache(maxsize=None)
def qkv_case(name, B, S, H, pre):
    """-> (dev, ref): dev fp32 [B, S, 3, H, 64] holding the bf16 values the kernel is fed (q multiplied by scale * log2e and re-rounded when
    pre), ref fp64 of the same shape: the unscaled q the kernel then effectively sees, k and v as they are"""
    gen = torch.Generator().manual_seed(64 * S + H + 7 * CASES.index(name))
    qkv = torch.randn(B, S, 3, H, HD, generator=gen)
    if name == "all_low":
        # every score of every row near -185 log2 units (q close to one direction u per head, k close to -16 u), a few nats apart: the keys
        # past S in a ragged tile score exactly 0 before they are masked, far ABOVE every real key.  A maximum taken before the mask moves the
        # reference to 0 and every exp2 underflows.
        u = torch.randn(1, 1, H, HD, generator=gen)
        u = 8.0 * u / u.norm(dim=-1, keepdim=True)
        qkv[:, :, 0] = u + 0.1 * qkv[:, :, 0]
        qkv[:, :, 1] = -16.0 * (u + 0.1 * qkv[:, :, 1])
        name = "randn"
    elif name == "early_giant":
        # key 3 x 40 in tile 0 (scores of +-60 .. 200 log2 units: rows it wins end tile 0 with a reference far above everything later), key 70
        # x 6 in tile 1 (makes the waves rescale there).  A rescale that may LOWER a reference multiplies those rows by exp2(+150).
        qkv[:, 3, 1] *= 40.0
        qkv[:, 70, 1] *= 6.0
        name = "randn"
    # staircase multiplies key 64 t + 17 by 3 (t + 1): past nine tiles (the chain shapes, S = 600 and 1100) the top steps would lead a row by
    # more than 100 nats -- a one-hot softmax that tests nothing.  There the steps are shrunk so that the last one is x 15.
    nt = (S + FK - 1) // FK
    scale_keys(qkv[:, :, 1], name, 5.0 / nt if name == "staircase" and nt > 9 else 1.0)
    qkv = rb(qkv)
    ref = qkv.double().clone()
    if pre:
        qkv = qkv.clone()
        qkv[:, :, 0] = rb(qkv[:, :, 0] * SC2)
        ref[:, :, 0] = qkv[:, :, 0].double() / SC2
    return qkv, ref


@functools.lru_cache(maxsize=None)
def grad_out(B, S, H):
    """the upstream gradient dO, fp32 [B, S, H * 64] holding bf16 values"""
    return rb(torch.randn(B, S, H * HD, generator=torch.Generator().manual_seed(5 + S + H)))


@functools.lru_cache(maxsize=None)
def reference(name, B, S, H, pre):
    """fp64 dense attention on qkv_case(...)'s ref: dict(o [B,S,H 64], lse2 [B,H,S] (log2 domain), dqkv [B,S,3,H,64] under grad_out,
    degenerate: rows whose best key leads by more than 100 nats).  Computed once per case; callers must not modify it."""
    _, ref = qkv_case(name, B, S, H, pre)
    o, lse2, s, g = dense_attention64(ref.reshape(B, S, 3 * H * HD), H, g=grad_out(B, S, H))
    degenerate = int(saturated_rows(s).sum()) if S > 1 else 0
    return dict(o=o, lse2=lse2, dqkv=g.reshape(B, S, 3, H, HD), degenerate=degenerate)


def lazy_policy64(qkv_dev, H, variant="m32"):
    """The reference policy of the pre-scaled hd64 forward in fp64, per (sample, head) and per wave of 32 query rows (rows past S repeat row
    S - 1, as the kernel clamps them).  qkv_dev: [B, S, 3, H, 64], q pre-scaled.
    -> dict(waves, tiles: key tiles per row, rescaled_waves: waves that took the rescale branch at some tile > 0, rescale_tiles: the set of
    tiles > 0 at which some wave did, stale_rows: live rows that at some tile > 0 kept a reference below the tile's maximum, max_stale_rise: the
    largest such rise (never above 8), m_final [B, H, S]: the reference each row ends with)"""
    B, S = qkv_dev.shape[:2]
    grp, ngrp = key_groups(variant)
    x = qkv_dev.double()
    s = torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1])                       # log2 units: q carries scale * log2e
    nt = (S + FK - 1) // FK
    s = torch.nn.functional.pad(s, (0, nt * FK - S), value=_NEG)
    nw = (S + WAVE_ROWS - 1) // WAVE_ROWS
    rows = torch.arange(nw * WAVE_ROWS).clamp_max(S - 1)
    live = (torch.arange(nw * WAVE_ROWS) < S).view(nw, WAVE_ROWS)
    s = s[:, :, rows].view(B, H, nw, WAVE_ROWS, nt, FK)
    m_run = torch.zeros(B, H, nw, WAVE_ROWS, dtype=torch.float64)
    rescaled = torch.zeros(B, H, nw, dtype=torch.bool)
    stale = torch.zeros(B, H, nw, WAVE_ROWS, dtype=torch.bool)
    rescale_tiles, max_rise = set(), 0.0
    for t in range(nt):
        st = s[..., t, :] - m_run[..., None]                                             # what the MFMA chain delivers: s - m_ref
        part = torch.stack([st[..., grp == g].max(-1).values for g in range(ngrp)], -1)  # the lanes' partial maxima  [B,H,nw,32,ngrp]
        take = (part > LAZY_THR).flatten(3).any(-1) if t else torch.ones(B, H, nw, dtype=torch.bool)
        mq = part.max(-1).values                                                         # the exchange: only where `take`
        delta = mq if t == 0 else mq.clamp_min(0.0)
        m_run = torch.where(take[..., None], m_run + delta, m_run)
        if t:
            rescaled |= take
            if bool(take.any()):
                rescale_tiles.add(t)
            rise = s[..., t, :].max(-1).values - m_run
            assert bool((rise <= LAZY_THR).all()), "a reference more than 8 below a tile maximum: the restatement is wrong"
            hit = (rise > 0) & live
            stale |= hit
            if bool(hit.any()):
                max_rise = max(max_rise, rise[hit].max().item())
    return dict(waves=B * H * nw, tiles=nt, rescaled_waves=int(rescaled.sum()), rescale_tiles=rescale_tiles, stale_rows=int(stale.sum()),
                max_stale_rise=max_rise, m_final=m_run.reshape(B, H, nw * WAVE_ROWS)[:, :, :S])


# ------------------------------------------------------------------------------------------------ small chains
# The backward gives every 256-key block of a (sample, head) to one workgroup ("item"), items in the order (sample, head, key block).  Its
# persistent grid has min(slots, items rounded up to 8) workgroups, slot = 8 XCDs x grid / 8 consecutive slots each; a slot sweeps the items
# slot, slot + grid, ... (one per generation).  Inside an XCD's slot range, runs of L slots aligned to multiples of L form a chain, cut at a
# head's last key block and at the end of the slot range; L is at most grid / 8 and at most the key blocks of a head.
#   name -> (B, H, S, chain_len knob, slots knob, expected (chain_len, grid, generations))
CHAIN_CASES = {
    # 3 key blocks x 6 heads = 18 items on a 24-slot grid, 3 slots per XCD: every head is one chain of 3 on one XCD, one generation
    "L3_one_generation": (1, 6, 600, 0, 0, (3, 24, 1)),
    # 48 items on 24 slots: every slot runs two key blocks, the counters go on counting in absolute steps across the generations
    "L3_two_generations": (2, 8, 600, 0, 24, (3, 24, 2)),
    # the same 18 items with chains of 2: key blocks 0 -> 1 chained, key block 2 on the last slot of the XCD range stands alone
    "L2": (1, 6, 600, 2, 0, (2, 24, 1)),
    # 5 key blocks x 7 heads = 35 items on 40 slots, 5 per XCD: key blocks 0 .. 3 one chain of 4, key block 4 cut off (range end and head end)
    "L4_with_cut": (1, 7, 1100, 4, 0, (4, 40, 1)),
}
CHAIN_FAMILIES = ("randn", "late_spike", "staircase")


def chain_plan_expected(name):
    return CHAIN_CASES[name][5]


def all_cases():
    """every (name, B, S, H) the GPU tests take a reference for (each both plain and pre-scaled unless noted there)"""
    out = [("randn", 2, S, 3) for S in FWD_EDGE_S]
    out += [(n, B, S, H) for n in SOFTMAX_CASES for B, H, S in FWD_LATE]
    out += [("late_spike", 2, S, 3) for S in FWD_SPIKE_S]
    out += [("randn", 2, 129, 5), ("randn", 2, 257, 3)]                                 # the two layout cases
    out += [("randn", 2, S, 2) for S in BWD_EDGE_S]
    out += [(n, B, S, H) for n in SOFTMAX_CASES for B, H, S in BWD_LATE]
    out += [(n, c[0], c[2], c[1]) for c in CHAIN_CASES.values() for n in CHAIN_FAMILIES]
    return sorted(set(out))
