"""World-2 rehearsal of reduce() -> clipped optimizer step on ONE card over gloo (the VT_DDP_BACKEND=gloo VT_ONE_GPU=1 set-up of
DESIGN 5), run by tests/test_grad_clip_gpu.py as one subprocess.

Without arguments this is the launcher: it imports nothing that opens the GPU, starts the two ranks as fresh interpreters, waits for
them under one deadline (a rank that fails or overstays takes the other down with it; nothing is retried) and prints ONE JSON line.
With ``--rank R`` it is a rank."""
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORLD, N, CLIP, LR, STEPS = 2, 300003, 0.5, 1e-2, 3
FACTORS = (8.0, 1.01, 0.5)          # norm of the MEAN gradient of each step, in units of CLIP: clips hard, barely, not at all


def launcher():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = tempfile.mkdtemp(prefix="grad_clip_ddp_")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(WORLD), LOCAL_RANK="0",
               VT_DDP_BACKEND="gloo", VT_ONE_GPU="1")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), "--out", out], env=dict(env, RANK=str(r)))
             for r in range(WORLD)]
    deadline, failed = time.time() + 300, None
    while failed is None and any(p.poll() is None for p in procs):
        if time.time() > deadline:
            failed = "deadline"
        elif any(p.poll() not in (None, 0) for p in procs):
            failed = "a rank failed"
        else:
            time.sleep(0.2)
    for p in procs:
        if p.poll() is None:
            p.kill()
        p.wait()
    codes = [p.returncode for p in procs]
    if failed is not None or any(codes):
        print(json.dumps({"error": failed or "a rank failed", "exit_codes": codes}))
        return 1
    ranks = [json.load(open(os.path.join(out, f"rank{r}.json"))) for r in range(WORLD)]
    import shutil
    shutil.rmtree(out, ignore_errors=True)
    print(json.dumps({"ranks": ranks}))
    return 0


def rank_main(rank: int, out: str):
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import hashlib
    from types import SimpleNamespace

    import torch
    from vt355.ddp import FlatGradReducer, init_from_env
    from vt355.optim import FusedAdamW

    r, _, world = init_from_env(os.environ["VT_DDP_BACKEND"])
    assert (r, world) == (rank, WORLD)
    dev = torch.device("cuda", 0)                                   # VT_ONE_GPU: both ranks share the card

    def state(seed):
        g = torch.Generator().manual_seed(seed)
        flat = torch.randn(N, generator=g).to(dev)
        bf = flat.to(torch.bfloat16)
        return SimpleNamespace(flat=flat, grad=torch.zeros(N, device=dev), flat_bf16=bf, params=[torch.nn.Parameter(bf)], version=0)

    def local_grads(step):
        """every rank can restate every rank's gradient (seeded); their mean has norm FACTORS[step] * CLIP"""
        gs = [torch.randn(N, generator=torch.Generator().manual_seed(1000 + 10 * step + k)).double() * (1.0 + k) for k in range(WORLD)]
        scale = FACTORS[step] * CLIP / (sum(gs) / WORLD).norm()
        return [(x * scale).float() for x in gs]

    st = state(7)
    opt = FusedAdamW(st.params, lr=LR, fullft_state=st, gradient_clip_val=CLIP)
    red = FlatGradReducer(st.grad)
    one = state(7)                                                  # the single-process step on the mean gradient
    ref = FusedAdamW(one.params, lr=LR, fullft_state=one, gradient_clip_val=CLIP)
    coef_bits, norm_bits, coefs, differ = [], [], [], True
    for step in range(STEPS):
        gs = local_grads(step)
        differ = differ and not torch.equal(gs[0], gs[1])
        st.grad.copy_(gs[rank])
        red.reduce()                                                # the all-reduce has FINISHED before the norm pass reads the sum
        opt.step(grad_scale=red.grad_scale)
        rec = opt._clip_record.clone()
        norm_bits.append(int(rec.view(torch.int32)[0].item())); coef_bits.append(int(rec.view(torch.int32)[1].item()))
        coefs.append(rec[1].item())
        one.grad.copy_(((gs[0].double() + gs[1].double()) / WORLD).float())
        ref.step()
    torch.cuda.synchronize()

    def out_of_tol(a, b, rtol, atol):
        a, b = a.float().cpu(), b.float().cpu()
        return ((a - b).abs() > atol + rtol * b.abs()).float().mean().item()

    sha = lambda *ts: hashlib.sha256(b"".join(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes() for t in ts)).hexdigest()
    res = dict(rank=rank, masters_sha256=sha(st.flat, st.flat_bf16), moments_sha256=sha(opt.m, opt.v), coef_bits=coef_bits,
               norm_bits=norm_bits, coefs=coefs, local_grads_differ=differ,
               out_of_tol_master=out_of_tol(st.flat, one.flat, 1e-5, 1e-6), out_of_tol_bf16=out_of_tol(st.flat_bf16, one.flat, 1e-2, 1e-3))
    with open(os.path.join(out, f"rank{rank}.json"), "w") as f:
        json.dump(res, f)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    if "--rank" in sys.argv:
        rank_main(int(sys.argv[sys.argv.index("--rank") + 1]), sys.argv[sys.argv.index("--out") + 1])
    else:
        sys.exit(launcher())
