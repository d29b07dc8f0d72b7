"""The relative-position temporal attention kernels of csrc/attn_relpos.hip alone, at the three temporal levels of the VideoCrafter1
recipe (configs/000_videocrafter/vc1_t2v_1024.yaml: batch 4, 72x128 latents, 16 frames, T = P = 16):

    R = 4*9216*16 rows, H = 5      R = 4*2304*16, H = 10      R = 4*576*16, H = 20

Forward and backward of
    relpos   vt_attn_relpos_fwd / _bwd (table gradients wanted: the full fine-tune's call)
    small    the shipped vt_attn_small masked kernels on the same q | k | v -- a LOWER BOUND: the same bytes, none of the table work
    torch    a torch-on-device restatement of the reference's einsum path (lvdm/modules/attention.py:126-149) in bf16, backward by autograd
One process, the variants alternating launch by launch; per variant the median and max - min of --launches HIP-event timings after
--warmup warm-up rounds.  "bytes" is what the algorithm must move (q, k, v read and o written; backward: q, k, v, o, dO read and dq, dk,
dv written), and GB/s is that over the median: a rate computed from shapes, not a counter reading.

    python tools/kbench_relpos.py [--launches 20] [--warmup 3] > profiles/relpos_kbench.txt
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS = [(4 * 9216 * 16, 5), (4 * 2304 * 16, 10), (4 * 576 * 16, 20)]
T = P = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--levels", default="0,1,2")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kbench_relpos needs an MI355X: a CPU run measures nothing")
    from vt355 import ops
    dev = torch.device("cuda:0")
    BF, F32 = torch.bfloat16, torch.float32
    g = torch.Generator(device=dev).manual_seed(0)
    for li in [int(v) for v in args.levels.split(",")]:
        R, H = LEVELS[li]
        D = H * 64
        qkv = torch.randn(R, 3 * D, device=dev, generator=g).to(BF)
        do = torch.randn(R, D, device=dev, generator=g).to(BF)
        ek = (torch.randn(2 * P + 1, 64, device=dev, generator=g) * 0.25).to(BF)
        ev = (torch.randn(2 * P + 1, 64, device=dev, generator=g) * 0.25).to(BF)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        o, o_s = torch.empty(R, D, dtype=BF, device=dev), torch.empty(R, D, dtype=BF, device=dev)
        lse, lse_s = torch.empty(H, R, dtype=F32, device=dev), torch.empty(1, H, R, dtype=F32, device=dev)
        dqkv = torch.empty(R, 3 * D, dtype=BF, device=dev)
        dek, dev_ = torch.zeros(2 * P + 1, 64, dtype=F32, device=dev), torch.zeros(2 * P + 1, 64, dtype=F32, device=dev)
        q3, k3, v3 = (t.unsqueeze(0) for t in (q, k, v))
        d3 = dqkv.unsqueeze(0)
        # the reference's path: (b h) n d layout, einsum -> softmax -> einsum, tables gathered per (i, j)
        idx = (torch.arange(T, device=dev)[None, :] - torch.arange(T, device=dev)[:, None]).clamp(-P, P) + P
        tq = qkv.detach().clone().requires_grad_(True)
        tek, tev = ek.clone().requires_grad_(True), ev.clone().requires_grad_(True)
        state = {}

        def torch_fwd():
            sp = lambda t: t.reshape(R // T, T, H, 64).permute(0, 2, 1, 3).reshape(-1, T, 64)
            tq_, tk_, tv_ = sp(tq[:, :D]), sp(tq[:, D:2 * D]), sp(tq[:, 2 * D:])
            sim = torch.einsum("bid,bjd->bij", tq_, tk_) * 0.125
            sim = sim + torch.einsum("btd,tsd->bts", tq_, tek[idx]) * 0.125
            sim = sim.softmax(dim=-1)
            out = torch.einsum("bij,bjd->bid", sim, tv_) + torch.einsum("bts,tsd->btd", sim, tev[idx])
            state["out"] = out.reshape(R // T, H, T, 64).permute(0, 2, 1, 3).reshape(R, D)

        def torch_bwd():
            tq.grad = tek.grad = tev.grad = None
            state["out"].backward(do, retain_graph=True)

        variants = {
            "fwd": [("relpos", lambda: ops.attn_relpos_fwd(q, k, v, ek, ev, o, lse, H, T, 0.125)),
                    ("small", lambda: ops.attn_small_fwd(q3, k3, v3, o_s.unsqueeze(0), lse_s, H, 0.125, mask_block=T)),
                    ("torch", torch_fwd)],
            "bwd": [("relpos", lambda: ops.attn_relpos_bwd(q, k, v, ek, ev, o, do, lse, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:], dek, dev_,
                                                          H, T, 0.125)),
                    ("small", lambda: ops.attn_small_bwd(q3, k3, v3, o_s.unsqueeze(0), do.unsqueeze(0), lse_s, d3[..., :D], d3[..., D:2 * D],
                                                         d3[..., 2 * D:], H, 0.125, mask_block=T)),
                    ("torch", torch_bwd)],
        }
        nbytes = {"fwd": 2.0 * 4 * R * D, "bwd": 2.0 * 8 * R * D}
        for direction in ("fwd", "bwd"):
            times = {n: [] for n, _ in variants[direction]}
            for it in range(args.warmup + args.launches):
                for name, fn in variants[direction]:            # alternating: every round times each variant once
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        times[name].append(e0.elapsed_time(e1))
            med = {n: statistics.median(ms) for n, ms in times.items()}
            for name, ms in times.items():
                print(json.dumps({"level": li, "R": R, "H": H, "T": T, "P": P, "pass": direction, "variant": name, "launches": len(ms),
                                  "median_ms": round(med[name], 4), "max_minus_min_ms": round(max(ms) - min(ms), 4),
                                  "algorithmic_GBps": round(nbytes[direction] / med[name] / 1e6, 1),
                                  "relpos_over_this": round(med["relpos"] / med[name], 3)}), flush=True)
        del qkv, do, o, o_s, dqkv, tq, state


if __name__ == "__main__":
    main()
